"""The deletion call on the GPU (vga_deletion_begin / _read / _reset / _end / _call / _call_table, k_dl_events + k_dl_keep + the
kernels of the call, `vgaligner map --call-variants --call-deletions`).  Every comparison is exact equality: the store's events,
element for element and in order, against the reference walker (tests/deletion_ref.py) run over the ORACLE's alignments GAF, on
every route a problem can take through poa_run; the calls against the reference's sort, grouping and rule; the TSV byte for byte
against the reference run on the run's own alignments GAF.  Without the feature every test here stops at Context.deletion_begin
(no such call) or at the unknown --call-deletions flag."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import deletion_cases
import deletion_ref
import op_cases as M
import pileup_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
W = deletion_ref.EVENT_WORDS


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


def oracle_gaf(oracle, ix, seqs, best_n=1):
    mp = oracle.default_map_params()
    mp.align_best_n = best_n
    return oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, mp)[1]


def walker(oracle, ix, seqs, best_n=1):
    """(events, n_alignments, n_end_runs) from the oracle's alignments GAF of seqs"""
    return deletion_ref.walk(oracle_gaf(oracle, ix, seqs, best_n), oracle_index_arrays(ix)["node_seq_idx"])


def same(got, want, what=""):
    print(what, "events", len(got[0]), "/", len(want[0]), "alignments", got[1], "/", want[1], "end runs", got[2], "/", want[2])
    assert got[1:] == want[1:], (what, "totals", got[1:], want[1:])
    g, w = got[0], want[0]
    assert g.dtype == np.uint32 and g.shape == w.shape and g.shape[1] == W, (what, g.shape, w.shape)
    bad = np.argwhere((g != w).any(1))[:, 0]
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def count(c, seqs, best_n=1, map_params=None):
    """one map + align call on a context that is storing"""
    b = c.batch(seqs)
    mo = b.map(map_params) if map_params is not None else b.map()
    al = b.align(mo, best_n=best_n)
    b.close()
    return al, mo


def fresh(c, ix):
    upload_oracle_index(c, ix)
    c.pileup_begin()
    c.deletion_begin()


def concat(x, y):
    return np.concatenate([x[0], y[0]]), x[1] + y[1], x[2] + y[2]


# ---- 1. the case sets
@pytest.fixture(scope="module")
def case_sets(oracle, tmp_path_factory):
    """name -> (case, oracle index, the reference's (events, n_alignments, n_end_runs)): the sets of deletion_cases and of op_cases"""
    tmp = tmp_path_factory.mktemp("dl_cases")
    out = {}
    for c in deletion_cases.all_cases(tmp) + M.all_cases(tmp):
        ix = oracle.Index(oracle.Graph.from_gfa(M.gfa_path(c, tmp)), c.k)
        out[c.name] = (c, ix, deletion_ref.walk(M.alignments(oracle, ix, c), oracle_index_arrays(ix)["node_seq_idx"]))
    return out


SETS = ("drb5-del-lanes", "drb5-del-blocks", "drb5-del-pairs", "drb1-del-ins", "drb1-del-nodes", "synth-del-nodes",
        "drb5-digits", "drb5-edges", "drb1-runs", "drb1-sweep", "drb1-entries", "synth-nodes", "drb1-both-strands")


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("env", [{}, {"VGA_DEL_LIST_WORDS": "0"}], ids=["lists on the device", "VGA_DEL_LIST_WORDS=0"])
def test_case_set(ctx, case_sets, monkeypatch, capfd, name, env):
    """a deletion list is three words per event: with the default buffer every list is k_dl_events' own, with no buffer the host's"""
    assert tuple(case_sets) == SETS
    p = pkg()
    c, ix, want = case_sets[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VGA_TRACE", "1")
    fresh(ctx, ix)
    capfd.readouterr()
    mp = p.default_map_params()
    if c.both_strands:
        mp.strands = p.binding.VGA_STRANDS_BOTH
    al, mo = count(ctx, c.reads, map_params=mp)
    by_host = len(re.findall(r"no room for its deletion list", capfd.readouterr().err))
    if c.both_strands:  # (a '-' record carries the forward path and the cs of the reverse complement)
        assert mo.strand.tolist() == [i % 2 for i in range(len(c.reads))]
    assert int(al.aligned.sum()) == len(c.reads) == want[1] <= al.poa_problems
    if not env:
        assert by_host == 0, by_host
        names = [t["name"] for t in ctx.kernel_times()]
        assert "k_dl_events" in names and "k_dl_keep" in names, names
    elif len(want[0]):
        assert 0 < by_host <= al.poa_problems
    same(ctx.deletions(), want, name + str(env))
    pu = ctx.pileup()[0]
    deletion_ref.check_against_pileup(ctx.deletions()[0], pu)
    # and the call, from the context's store and counters, against the reference on the reference's events and this pileup
    for thresholds in ((deletion_ref.ERROR, 1, 0), (deletion_ref.ERROR, deletion_ref.MIN_DEPTH, deletion_ref.MIN_QUAL)):
        assert deletion_ref.same(ctx.deletion_call(*thresholds), deletion_ref.call(want[0], pu, *thresholds)) is None, thresholds
    ctx.pileup_end()


# ---- 2. the routes
@pytest.fixture(scope="module")
def routes(oracle, drb1):
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 8, 2500, 0.03, 0.03, 0.04, seed=12)]
    want = walker(oracle, drb1, seqs)
    assert want[1] == len(seqs) and len(want[0]) > 300
    return seqs, want


@pytest.mark.parametrize("env", [{}, {"VGA_DEL_LIST_WORDS": "0"}, {"VGA_DEL_LIST_WORDS": "400"}, {"VGA_POA_KERNEL": "t6"}, {"VGA_POA_KERNEL": "t7"},
                                 {"VGA_POA_TEXT": "host"}, {"VGA_DEL_LIST_WORDS": "400", "VGA_POA_TEXT": "host"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "defaults")
def test_routes_store_the_same(ctx, drb1, routes, monkeypatch, capfd, env):
    """forced DP kernels (t6 hands wide problems back: a problem that runs twice replaces its record), text on the host, and a list
    buffer too small for all problems or for any: the host builds the lists that found no room"""
    seqs, want = routes
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VGA_TRACE", "1")
    fresh(ctx, drb1)
    capfd.readouterr()
    al, _ = count(ctx, seqs)
    trace = capfd.readouterr().err
    same(ctx.deletions(), want, str(env))
    ctx.pileup_end()
    by_host = len(re.findall(r"no room for its deletion list", trace))
    print("problems", al.poa_problems, "lists built by the host", by_host)
    words = env.get("VGA_DEL_LIST_WORDS")
    if words == "0":
        assert by_host == al.poa_problems == len(seqs)
    elif words is not None:
        assert 0 < by_host < al.poa_problems, "some lists on the device, some built by the host"
    else:
        assert by_host == 0


def test_best_of_two_candidates(oracle, ctx, drb1, monkeypatch):
    """only the reported record of a read is kept"""
    src = pkg().readsim.simulate_reads(DRB1, 6, 700, 0.02, 0.02, 0.02, seed=23)
    seqs = [r.seq[:500] + r.seq[:500] for r in src] + [src[0].seq[:300] * 3, src[1].seq]
    monkeypatch.setenv("VGA_POA_SUB", "2")  # (two problems per launch: a read's candidates fall into different ones)
    fresh(ctx, drb1)
    al, mo = count(ctx, seqs, best_n=2)
    assert max(len(mo.chains_of(r)) for r in range(len(seqs))) >= 2 and al.poa_problems > len(seqs)
    same(ctx.deletions(), walker(oracle, drb1, seqs, 2), "best_n 2")
    ctx.pileup_end()


# ---- 3. life cycle: two batches, a reset, the store that doubles, what ends it
def test_life_cycle(oracle, drb1, monkeypatch, capfd):
    p = pkg()
    s1 = [r.seq for r in p.readsim.simulate_reads(DRB1, 10, 2000, 0.03, 0.03, 0.04, seed=51)]
    s2 = [r.seq for r in p.readsim.simulate_reads(DRB1, 7, 1500, 0.03, 0.03, 0.04, seed=52)] + ["ACGT" * 30]
    w1, w2 = walker(oracle, drb1, s1), walker(oracle, drb1, s2)
    assert w2[1] == 7  # (the last read has no chain: a placeholder record adds nothing)
    c = p.Context(0)
    try:
        with pytest.raises(p.VgaError) as e:
            c.deletion_begin()
        assert e.value.code == -5  # VGA_ERR_NO_INDEX
        upload_oracle_index(c, drb1)
        with pytest.raises(p.VgaError) as e:
            c.deletion_begin()
        assert e.value.code == -1 and "vga_pileup_begin" in str(e.value)  # begin comes after vga_pileup_begin
        c.pileup_begin()
        for call in (c.deletions, c.deletion_reset, c.deletion_call):
            with pytest.raises(p.VgaError) as e:
                call()
            assert e.value.code == -1  # VGA_ERR_ARG: read / reset / call before begin
        count(c, s1)
        assert not any(t["name"].startswith("k_dl") for t in c.kernel_times()), "the store off: no deletion kernel"
        c.deletion_begin()
        count(c, s1)
        same(c.deletions(), w1, "first call")
        same(c.deletions(), w1, "read twice")
        count(c, s2)
        same(c.deletions(), concat(w1, w2), "two calls: the second behind the first")
        c.deletion_reset()
        events, n, ends = c.deletions()
        assert (len(events), n, ends) == (0, 0, 0)
        assert c.deletion_call(deletion_ref.ERROR, 1, 0)["n_distinct"] == 0
        count(c, s2)
        same(c.deletions(), w2, "after reset")
        c.deletion_begin()   # begin again empties
        assert c.deletions()[1:] == (0, 0)
        # subgraphs on the host are refused while the store is on
        monkeypatch.setenv("VGA_SUBGRAPH", "host")
        with pytest.raises(p.VgaError) as e:
            count(c, s2)
        assert e.value.code == -4 and "VGA_SUBGRAPH" in str(e.value)
        monkeypatch.delenv("VGA_SUBGRAPH")
        # vga_pileup_end drops the store
        c.pileup_end()
        with pytest.raises(p.VgaError) as e:
            c.deletions()
        assert e.value.code == -1
        # ... and so does a new index
        c.pileup_begin()
        c.deletion_begin()
        upload_oracle_index(c, drb1)
        with pytest.raises(p.VgaError) as e:
            c.deletions()
        assert e.value.code == -1
        count(c, s1)
        assert not any(t["name"].startswith("k_dl") for t in c.kernel_times())
        c.deletion_end()
        c.deletion_end()  # (ending twice is harmless)
    finally:
        c.close()


@pytest.fixture(scope="module")
def drb1_300(oracle, drb1):
    """300 reads of DRB1, the oracle's alignments GAF of them and the reference's events"""
    reads = pkg().readsim.simulate_reads(DRB1, 300, 400, 0.02, 0.01, 0.01, seed=61)
    _, gaf, _ = oracle.map_reads(drb1, [r.name for r in reads], [r.seq for r in reads])
    return reads, gaf, deletion_ref.walk(gaf, oracle_index_arrays(drb1)["node_seq_idx"])


def test_the_store_doubles(ctx, drb1, drb1_300, monkeypatch, capfd):
    """300 reads in batches of 100 pass the store's first size (DELETION_STORE_EVENTS0 events): it doubles at least once with
    events in it, and nothing is lost or reordered"""
    reads, gaf, want = drb1_300
    first = pkg().binding.DELETION_STORE_EVENTS0
    assert len(want[0]) > first, (len(want[0]), first)
    monkeypatch.setenv("VGA_TRACE", "1")
    fresh(ctx, drb1)
    capfd.readouterr()
    for at in range(0, 300, 100):
        count(ctx, [r.seq for r in reads[at:at + 100]])
    grown = re.findall(r"deletions: the store grows from (\d+) to (\d+) words", capfd.readouterr().err)
    print(grown)
    assert grown and int(grown[0][0]) == 0 and int(grown[0][1]) == first * W
    assert [g for g in grown if int(g[0]) > 0], "a doubling that moves what is stored"
    same(ctx.deletions(), want, "300 reads in three calls")
    ctx.pileup_end()


def test_switch_off_launches_nothing(ctx, drb1, routes):
    upload_oracle_index(ctx, drb1)
    ctx.pileup_begin()
    count(ctx, routes[0])
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_pu_events" in names and not [n for n in names if n.startswith("k_dl")], names
    ctx.pileup_end()


# ---- 4. the seam
N_BASES = 70000


def table(n_bases, seed):
    """a pileup table with zero rows, shallow rows, deep rows and counters just below 2^40"""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 2, size=(n_bases, 7)).astype(np.uint64)
    t[::5] = rng.integers(0, 60, size=(len(t[::5]), 7))
    t[::11] = 0
    t[3::97] = rng.choice(np.array([0, 2**32 - 1, 2**32, 2**40 - 1], dtype=np.uint64), size=(len(t[3::97]), 7))
    return t


def random_events(n, seed, n_bases=N_BASES):
    """events drawn from a small pool (groups of many sizes) among unique ones"""
    rng = np.random.default_rng(seed)
    pool = np.stack([rng.integers(0, n_bases, 40), rng.integers(1, 30, 40), rng.integers(0, n_bases, 40)], 1)
    ev = np.stack([rng.integers(0, n_bases, n), rng.integers(1, 3000, n), rng.integers(0, n_bases, n)], 1)
    pick = rng.random(n) < 0.6
    ev[pick] = pool[rng.integers(0, 40, int(pick.sum()))]
    return ev.astype(np.uint32)


def seam(ctx, ev, tab, *thresholds, **kw):
    got = ctx.deletion_call_table(ev, tab, *thresholds, **kw)
    want = deletion_ref.call(ev, tab, *thresholds)
    bad = deletion_ref.same(got, want)
    assert bad is None, (bad, np.asarray(got[bad]).tolist()[:6], np.asarray(want[bad]).tolist()[:6])
    return got


@pytest.fixture(scope="module")
def tab():
    return table(N_BASES, 3)


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 4095, 4096, 4097])
def test_seam_at_the_scan_block_and_radix_tile_edges(ctx, tab, n):
    got = seam(ctx, random_events(n, 100 + n), tab, deletion_ref.ERROR, 1, 0)
    assert got["n_calls"] > 0 or n < 2
    seam(ctx, random_events(n, 200 + n), tab)
    names = [t["name"] for t in ctx.kernel_times()]
    assert ("k_dl_group" in names and "k_dl_sort_first" in names) == (n > 0), names


def test_seam_groups(ctx, tab):
    deep, one = np.full((N_BASES, 7), 2, dtype=np.uint64), np.zeros((N_BASES, 7), dtype=np.uint64)
    one[:, 2] = 1   # depth 1: a single read is called hom, so every group is reported
    # all events identical
    got = seam(ctx, np.array([[77, 5, 81]] * 5000, dtype=np.uint32), deep, deletion_ref.ERROR, 1, 0)
    assert (got["n_distinct"], got["n_calls"], got["reads"].tolist(), got["depth"].tolist()) == (1, 1, [5000], [12])
    # all distinct
    ev = np.stack([np.arange(5000) * 13 % N_BASES, np.arange(5000) % 7 + 1, np.arange(5000)], 1).astype(np.uint32)
    got = seam(ctx, ev[np.random.default_rng(1).permutation(5000)], one, deletion_ref.ERROR, 1, 0)
    assert got["n_distinct"] == 5000 and set(got["reads"].tolist()) == {1}
    # a group that straddles a tile edge of the sorted order: 4090 smaller keys, then 12 equal ones, then more
    ev = np.concatenate([np.stack([np.arange(4090), np.ones(4090), np.arange(4090)], 1), [[5000, 2, 5001]] * 12,
                         np.stack([np.arange(6000, 6300), np.ones(300), np.arange(6000, 6300)], 1)]).astype(np.uint32)
    got = seam(ctx, ev[np.random.default_rng(2).permutation(len(ev))], one, deletion_ref.ERROR, 1, 0)
    assert got["reads"].tolist()[4090] == 12 and got["n_distinct"] == 4090 + 1 + 300


def test_seam_keys_that_differ_in_one_field(ctx, tab):
    """only in last, only in len, only in the third byte of first, and a len above 2^16: each is a group of its own, in order"""
    deep = np.zeros((N_BASES, 7), dtype=np.uint64)
    deep[:, 5] = 1   # depth 1: a single read is called hom, so every group is reported
    ev = np.array([[300, 4, 900], [300, 4, 303], [300, 4, 900],            # last
                   [300, 5, 900], [300, 4, 900],                            # len
                   [0x10000 + 300, 4, 900], [300, 4, 900], [0x10000 + 300, 4, 900],   # the third byte of first
                   [300, 0x10000 + 4, 900], [300, 0x12345, 69999], [300, 2**32 - 1, 900]], dtype=np.uint32)   # len above 2^16
    got = seam(ctx, ev, deep, deletion_ref.ERROR, 1, 0)
    assert list(zip(got["first"].tolist(), got["len"].tolist(), got["last"].tolist(), got["reads"].tolist())) == [
        (300, 4, 303, 1), (300, 4, 900, 4), (300, 5, 900, 1), (300, 0x10004, 900, 1), (300, 0x12345, 69999, 1), (300, 2**32 - 1, 900, 1), (0x10000 + 300, 4, 900, 2)]
    # positions up to the last base, and a table of one base
    seam(ctx, np.array([[N_BASES - 1, 1, N_BASES - 1], [0, 3, N_BASES - 1], [N_BASES - 1, 2, 0]], dtype=np.uint32), deep, deletion_ref.ERROR, 1, 0)
    seam(ctx, np.array([[0, 1, 0]] * 3, dtype=np.uint32), deep[:1], deletion_ref.ERROR, 1, 0)


def test_seam_cap(ctx, tab):
    """cap 0 and cap one below n_calls: the counts come back whole and nothing is written beyond cap"""
    ev = random_events(3000, 7)
    want = deletion_ref.call(ev, tab, deletion_ref.ERROR, 1, 0)
    n = want["n_calls"]
    assert n > 100
    for cap in (0, n - 1, n, n + 5):
        got = ctx.deletion_call_table(ev, tab, deletion_ref.ERROR, 1, 0, cap=cap, ask_again=False)
        assert (got["n_distinct"], got["n_calls"]) == (want["n_distinct"], n) and len(got["first"]) == min(cap, n)
        assert deletion_ref.same(got, want, upto=min(cap, n)) is None, cap
    # the raw call: the arrays behind cap keep what they held
    L, m = ctx.L, n - 1
    u32 = lambda: np.full(n + 4, 0xABCDABCD, dtype=np.uint32)
    first, length, last, qual = u32(), u32(), u32(), u32()
    state, depth, reads = np.full(n + 4, 0xEE, dtype=np.uint8), np.full(n + 4, 7, dtype=np.uint64), np.full(n + 4, 7, dtype=np.uint64)
    nd, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    t64 = np.ascontiguousarray(tab)
    rc = L.vga_deletion_call_table(ctx.h, len(ev), P(ev, ctypes.c_uint32), len(t64), P(t64, ctypes.c_uint64), deletion_ref.ERROR, 1, 0, m, P(first, ctypes.c_uint32),
                                   P(length, ctypes.c_uint32), P(last, ctypes.c_uint32), P(state, ctypes.c_uint8), P(qual, ctypes.c_uint32), P(depth, ctypes.c_uint64),
                                   P(reads, ctypes.c_uint64), ctypes.byref(nd), ctypes.byref(nc))
    assert rc == 0 and nc.value == n
    assert np.array_equal(first[:m], want["first"][:m]) and np.array_equal(reads[:m], want["reads"][:m])
    assert (first[m:] == 0xABCDABCD).all() and (qual[m:] == 0xABCDABCD).all() and (state[m:] == 0xEE).all() and (depth[m:] == 7).all() and (reads[m:] == 7).all()


def test_seam_refusals(ctx, tab):
    p = pkg()
    ok = np.array([[5, 2, 6], [9, 1, 9]], dtype=np.uint32)
    small = tab[:100]

    def refused(code, ev=ok, t=small, *a, **kw):
        with pytest.raises(p.VgaError) as e:
            ctx.deletion_call_table(ev, t, *a, **kw)
        assert e.value.code == code, (e.value.code, str(e.value))

    for bad in ([100, 1, 5], [5, 1, 100], [5, 0, 6], [2**32 - 1, 1, 5]):   # first, last below n_bases; len at least 1
        refused(-1, np.array([[5, 2, 6], bad], dtype=np.uint32))
    refused(-1, ok, small[:0])                       # no base at all holds no event
    for error in (256, 8193):
        refused(-1, ok, small, error)                # the parameter ranges of vga_variant_call
    refused(-1, ok, small, deletion_ref.ERROR, 0)
    seam(ctx, ok, small, 257, 1, 0)
    seam(ctx, ok, small, 8192, 1, 2**63)
    # 2^32 - 1 events or more, 2^31 bases or more: refused before anything is read (so a short array will do)
    L = ctx.L
    P = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    one, row = np.zeros(3, dtype=np.uint32), np.zeros(7, dtype=np.uint64)
    nd, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    tail = (deletion_ref.ERROR, 1, 0, 0, None, None, None, None, None, None, None, ctypes.byref(nd), ctypes.byref(nc))
    assert L.vga_deletion_call_table(ctx.h, 2**32 - 1, P(one, ctypes.c_uint32), 1, P(row, ctypes.c_uint64), *tail) == -4   # VGA_ERR_UNSUPPORTED
    assert L.vga_deletion_call_table(ctx.h, 0, P(one, ctypes.c_uint32), 2**31, P(row, ctypes.c_uint64), *tail) == -4
    assert L.vga_deletion_call_table(ctx.h, 1, None, 1, P(row, ctypes.c_uint64), *tail) == -1                               # a null array
    assert L.vga_deletion_call_table(ctx.h, 0, None, 0, None, deletion_ref.ERROR, 1, 0, 3, None, None, None, None, None, None, None, None, None) == -1
    # a counter of 2^40 or more at the first base of an event (found on the device)
    for col in (0, 5):
        wide = small.copy()
        wide[5, col] = 2**40
        refused(-4, ok, wide)
        wide[5, col] = 2**40 - 1
        seam(ctx, ok, wide, deletion_ref.ERROR, 1, 0)
    wide = small.copy()
    wide[5, 6] = 2**40   # (the ins column is not part of the depth)
    seam(ctx, ok, wide, deletion_ref.ERROR, 1, 0)


# ---- 5. the context against the seam against the executable
def write_fasta(path, reads):
    with open(path, "w") as f:
        for name, seq in reads:
            f.write(">%s\n%s\n" % (name, seq))


@pytest.fixture(scope="module")
def samples(oracle, drb1, drb1_300):
    a = oracle_index_arrays(drb1)
    nid, site, planted = deletion_cases.planted_reads(a["node_seq_idx"])
    return {"drb1-300": [(r.name, r.seq) for r in drb1_300[0]], "planted-hom": planted["hom"], "planted-het": planted["het"]}, nid, site


@pytest.mark.parametrize("sample", ["drb1-300", "planted-hom", "planted-het"])
def test_context_seam_and_cli_agree(oracle, ctx, drb1, samples, tmp_path, sample):
    p = pkg()
    reads = samples[0][sample]
    a = oracle_index_arrays(drb1)
    _, oag, _ = oracle.map_reads(drb1, [n for n, _ in reads], [s for _, s in reads])
    want_text, want_message, want = deletion_ref.tsv_gaf(oag, a["node_seq_idx"], a["seq_fwd"])
    # the context's route and the seam
    fresh(ctx, drb1)
    count(ctx, [s for _, s in reads])
    events, n_al, n_end = ctx.deletions()
    same((events, n_al, n_end), deletion_ref.walk(oag, a["node_seq_idx"]), sample)
    pu = ctx.pileup()[0]
    assert np.array_equal(pu, pileup_ref.walk(oag, a["node_seq_idx"], a["seq_fwd"])[0])
    got = ctx.deletion_call()
    assert deletion_ref.same(got, want) is None
    assert deletion_ref.same(ctx.deletion_call_table(events, pu), want) is None
    assert deletion_ref.same(ctx.deletion_call(cap=0), want) is None, "asks again by itself"
    assert np.array_equal(ctx.deletions()[0], events), "the call does not reset or reorder the store"
    ctx.pileup_end()
    if sample.startswith("planted"):
        big = [i for i, r in enumerate(got["reads"].tolist()) if r >= 6]
        assert len(big) == 1 and int(got["first"][big[0]]) == samples[2] and int(got["len"][big[0]]) == deletion_cases.PLANTED
        assert deletion_ref.STATES[int(got["state"][big[0]])] == sample[-3:] and int(got["reads"][big[0]]) == 11
    # the executable, with one context and with several
    d = str(tmp_path)
    fa = os.path.join(d, "r.fa")
    write_fasta(fa, reads)

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    read = lambda name: open(os.path.join(d, name)).read()
    for out, extra in (("one", []), ("two", ["--devices", "0,0", "--chunk-reads", "7"])):
        run(common + ["-o", os.path.join(d, out + "-off"), "--call-variants"] + extra)
        assert not os.path.exists(os.path.join(d, out + "-off-deletions.tsv"))
        assert read(out + "-off-alignments.gaf") == oag
        pr = run(common + ["-o", os.path.join(d, out + "-on"), "--call-variants", "--call-deletions"] + extra)
        own_text, own_message, _ = deletion_ref.tsv_gaf(read(out + "-on-alignments.gaf"), a["node_seq_idx"], a["seq_fwd"])
        assert read(out + "-on-deletions.tsv") == own_text == want_text, out
        assert own_message == want_message and want_message in pr.stderr, (want_message, pr.stderr)
        # every other file is byte for byte what it is without the switch
        on = {f[len(out + "-on"):] for f in os.listdir(d) if f.startswith(out + "-on-")}
        assert on == {f[len(out + "-off"):] for f in os.listdir(d) if f.startswith(out + "-off-")} | {"-deletions.tsv"}
        for suffix in on - {"-deletions.tsv"}:
            assert read(out + "-on" + suffix) == read(out + "-off" + suffix), (out, suffix)


def test_cli_writes_the_header_alone_without_a_call(drb1, tmp_path):
    d = str(tmp_path)
    reads = pkg().readsim.simulate_reads(DRB1, 3, 400, 0.0, 0.0, 0.0, seed=5)
    fa = os.path.join(d, "r.fa")
    write_fasta(fa, [(r.name, r.seq) for r in reads])
    for args in (["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")],
                 ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1, "-o", os.path.join(d, "o"), "--call-variants",
                  "--call-deletions"]):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
    assert open(os.path.join(d, "o-deletions.tsv")).read() == deletion_ref.HEADER + "\n"
    assert re.search(r"call-deletions: \d+ runs of 3 alignments, \d+ at an end, \d+ distinct, 0 calls", pr.stderr), pr.stderr
    pr = subprocess.run([EXE, "map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1, "-o", os.path.join(d, "bad"), "--call-deletions"],
                        cwd=d, capture_output=True, text=True, timeout=300)
    assert pr.returncode != 0 and "--call-variants" in pr.stderr and not [f for f in os.listdir(d) if f.startswith("bad")]
