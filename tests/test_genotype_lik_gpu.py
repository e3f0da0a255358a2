"""The diploid read likelihood on the GPU (vga_genotype_lik_begin / _read / _reset / _end / _pairs, k_gl_deficit, k_gl_pairs,
`vgaligner map --genotype-likelihood`).  Every comparison is exact equality of integer arrays -- cost, deficit, n_scored -- with
tests/genotype_lik_ref.py on the library's table: through the kernel seam over explicit matrices, and end to end over the matrices
the reference walker (tests/path_support_ref.py) gives for the ORACLE's alignments GAF.  Without the feature every test here stops
at Context.genotype_likelihood_pairs / genotype_likelihood_begin (no such call) or at the unknown --genotype-likelihood flag."""
import os
import subprocess

import numpy as np
import pytest

import coverage_ref
import genotype_lik_ref as ref
import genotype_ref
import path_support_ref
import pileup_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
LAM, CAP = 512, 64
KERNELS = ["k_gl_deficit", "k_gl_pairs"]
_tables = {}


def table(lam=LAM, cap=CAP):
    if (lam, cap) not in _tables:
        _tables[(lam, cap)] = pkg().binding.genotype_likelihood_table(lam, cap)
    return _tables[(lam, cap)]


def want_of(b, e, lam=LAM, cap=CAP):
    return ref.pairs(b, e, lam, cap, table(lam, cap))


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


# =====================================================================================================================
# 1. the kernel seam
# =====================================================================================================================
def matrices(rng, n_reads, n_paths, spread):
    """rows whose s lie within `spread` of each other around a per-row level, so that deficits fall on both sides of the cap"""
    level = rng.integers(0, 1 << 17, (n_reads, 1), dtype=np.int64) + spread
    s = level - rng.integers(0, spread + 1, (n_reads, n_paths), dtype=np.int64)
    e = rng.integers(0, 40, (n_reads, n_paths), dtype=np.int64)
    e = np.minimum(e, s)
    return (s - e).astype(np.uint32), e.astype(np.uint32)


def seam_path_counts():
    T = pkg().binding.GENOTYPE_LIK_TILE  # (the sizes the issue names, and the tile's own edges)
    return sorted({1, 2, 3, 63, 64, 65, 129, T - 1, T, T + 1, 2 * T + 1})


@pytest.mark.parametrize("n_paths", seam_path_counts())
def test_seam_tile_and_chunk_edges(ctx, n_paths):
    """a tile that is not full, exactly full, one path into the next tile, a diagonal and an off-diagonal tile, a wave of
    k_gl_deficit that is not full, full, and one path into its next round; no read, one, a chunk that is not full, full, one read into
    the next, two chunks and one.  A quarter of the cells repeat the cell of the path before (ties)"""
    R = pkg().binding.GENOTYPE_LIK_READS
    rng = np.random.default_rng(2000 + n_paths)
    for n_reads in sorted({0, 1, 31, 32, 33, 65, R - 1, R, R + 1, 2 * R + 1}):
        b, e = matrices(rng, n_reads, n_paths, 2 * CAP)
        if n_paths > 1 and n_reads:
            tie = rng.random((n_reads, n_paths - 1)) < 0.25
            b[:, 1:][tie] = b[:, :-1][tie]
            e[:, 1:][tie] = e[:, :-1][tie]
        got = ctx.genotype_likelihood_pairs(b, e, LAM, CAP)
        ref.same(got, want_of(b, e), "n_paths %d n_reads %d" % (n_paths, n_reads))
        if n_reads == 0:
            assert not got["cost"].any() and got["n_scored"] == 0 and got["deficit"].shape == (0, n_paths)
            assert ctx.kernel_times() == []
    names = [t["name"] for t in ctx.kernel_times()]
    assert names == KERNELS, names


def test_seam_every_difference_at_the_largest_cap(ctx):
    """cap = 255: path 0 holds the maximum, path 1 a deficit x and path 2 a deficit y, over rows that give every |x - y| from 0 to 255
    (and every min) between paths 1 and 2, and every x against the 0 of path 0"""
    x = np.arange(256)
    d1 = np.concatenate([x, np.full(256, 255), x, 255 - x])
    d2 = np.concatenate([np.zeros(256, dtype=np.int64), 255 - x, x, x])
    s = np.stack([np.full(len(d1), 1000), 1000 - d1, 1000 - d2], axis=1)
    assert set(np.abs(d1 - d2).tolist()) == set(range(256))
    b, e = (s // 2).astype(np.uint32), (s - s // 2).astype(np.uint32)
    for lam in (1, 512, 4096):
        want = want_of(b, e, lam, 255)
        assert want["deficit"][:, 1].tolist() == d1.tolist() and want["deficit"][:, 2].tolist() == d2.tolist()
        ref.same(ctx.genotype_likelihood_pairs(b, e, lam, 255), want, "every difference, lambda %d" % lam)


@pytest.mark.parametrize("cap", [1, 2, 64, 254, 255])
def test_seam_deficits_straddle_the_cap(ctx, cap):
    rng = np.random.default_rng(40 + cap)
    n_reads, n_paths = 70, 37
    s = np.full((n_reads, n_paths), 5000, dtype=np.int64) - rng.integers(max(0, cap - 3), cap + 4, (n_reads, n_paths))
    s[np.arange(n_reads), rng.integers(0, n_paths, n_reads)] = 5000  # (the row's maximum)
    b = rng.integers(0, 3000, s.shape)
    want = want_of(b, s - b, 300, cap)
    d = want["deficit"]
    assert d.max() == cap and (d == cap).sum() > 100 and (cap == 1 or (d == cap - 1).sum() > 100)
    ref.same(ctx.genotype_likelihood_pairs(b.astype(np.uint32), (s - b).astype(np.uint32), 300, cap), want, "cap %d" % cap)


@pytest.mark.parametrize("n_paths", [65, 130, 200])
def test_seam_where_the_maximum_sits(ctx, n_paths):
    """the row maximum in the last path, in the first path of the last partial tile (of 64 lanes for k_gl_deficit, of the tile for
    k_gl_pairs), and in the first path; every other row is huge at its front, which is what a lane past the end of the row before
    it would read: masked lanes must not win the maximum"""
    T = pkg().binding.GENOTYPE_LIK_TILE
    rng = np.random.default_rng(n_paths)
    spots = sorted({n_paths - 1, (n_paths - 1) // 64 * 64, (n_paths - 1) // T * T, 0, 63 % n_paths})
    n_reads = 2 * len(spots) + 1
    b = rng.integers(0, 50, (n_reads, n_paths)).astype(np.uint32)
    e = rng.integers(0, 50, (n_reads, n_paths)).astype(np.uint32)
    b[0::2] = 0xFFFFFF00  # rows 0, 2, ..: huge everywhere, above all at the front
    b[0::2, :8] = 0xFFFFFFFF
    for k, at in enumerate(spots):
        b[2 * k + 1, at] = 130  # rows 1, 3, ..: small, the maximum at one known spot
    want = want_of(b, e)
    for k, at in enumerate(spots):
        assert want["deficit"][2 * k + 1, at] == 0 and (want["deficit"][2 * k + 1] == 0).sum() == 1
        assert want["deficit"][2 * k + 1].min() == 0 and want["deficit"][2 * k + 1].max() <= CAP
    ref.same(ctx.genotype_likelihood_pairs(b, e), want, "maximum at %r of %d" % (spots, n_paths))


def test_seam_s_above_32_bits(ctx):
    b = np.zeros((4, 5), dtype=np.uint32)
    e = np.zeros((4, 5), dtype=np.uint32)
    b[:, 1] = e[:, 1] = 0xFFFFFFFF   # s = 2^33 - 2 beside zeros
    b[1, 3] = 0xFFFFFFFF
    e[1, 3] = 0xFFFFFFFE              # one below
    b[2, 2] = 0xFFFFFFFF              # s = 2^32 - 1: 2^32 - 1 below, where 32-bit arithmetic would see a deficit of 1
    e[2, 2] = 0
    b[3] = e[3] = 0                   # an all-zero row
    want = want_of(b, e)
    assert want["deficit"].tolist() == [[CAP, 0, CAP, CAP, CAP], [CAP, 0, CAP, 1, CAP], [CAP, 0, CAP, CAP, CAP], [0] * 5] and want["n_scored"] == 3
    ref.same(ctx.genotype_likelihood_pairs(b, e), want, "s above 32 bits")


def test_seam_total_above_32_bits(ctx):
    """5 000 reads at lambda = 4096, cap = 255 with every deficit but the maximum's at the cap: the pair (1, 1) of two paths, and (1, 2)
    of three, cost 5 000 * 4096 * 255 > 2^32"""
    n = 5000
    for n_paths in (2, 3):
        b = np.zeros((n, n_paths), dtype=np.uint32)
        e = np.zeros((n, n_paths), dtype=np.uint32)
        b[:, 0] = 700
        e[:, 0] = 300
        b[::2, 1:] = 400  # (half the rows 600 below, half 1 000 below: both past the cap)
        want = want_of(b, e, 4096, 255)
        assert int(want["cost"][ref.pair_index(n_paths, 1, n_paths - 1)]) == n * 4096 * 255 > 1 << 32
        assert int(want["cost"][ref.pair_index(n_paths, 0, 1)]) == n * int(table(4096, 255)[255])
        ref.same(ctx.genotype_likelihood_pairs(b, e, 4096, 255), want, "%d paths" % n_paths)


def test_seam_reads_split_over_workgroups(ctx):
    """12 paths are one tile: 5 125 reads are more than GENOTYPE_LIK_MIN_CHUNKS chunks and are split over workgroups, which atomics
    combine"""
    b_ = pkg().binding
    n_reads = 5125
    assert n_reads > 2 * b_.GENOTYPE_LIK_MIN_CHUNKS * b_.GENOTYPE_LIK_READS
    b, e = matrices(np.random.default_rng(7), n_reads, 12, 90)
    b[::7] = 0
    e[::7] = 0  # rows that are all zero cost nothing and are not scored
    want = want_of(b, e)
    assert want["n_scored"] == n_reads - len(b[::7])
    ref.same(ctx.genotype_likelihood_pairs(b, e), want, "split")


def test_seam_more_reads_than_a_workgroup_s_accumulators_hold(ctx):
    """with 32 tiles on a side there are so many tiles that the rule of gt_groups alone gives a workgroup half of the 6 144 reads;
    at lambda = 4096 and cap = 255, with most deficits at the cap, 32-bit accumulators that hold twice the cost overflow beyond
    2 055 such reads, so the cost is right only if the reads are split at GENOTYPE_LIK_MAX_GROUP_READS.  Three kinds of rows repeat,
    so the reference is three rows"""
    b_ = pkg().binding
    n_paths = 31 * b_.GENOTYPE_LIK_TILE + 1
    n_reads = 3 * b_.GENOTYPE_LIK_MAX_GROUP_READS
    rng = np.random.default_rng(11)
    kinds_b = np.zeros((3, n_paths), dtype=np.uint32)
    kinds_b[0, 0] = 1000                                     # one path at the maximum, all others at the cap
    kinds_b[1] = rng.integers(0, 2, n_paths) * 1000          # half at the maximum, half at the cap
    kinds_b[2] = 1000 - rng.integers(0, 256, n_paths)        # every deficit
    kinds_b[2, 5] = 1000
    which = np.arange(n_reads) % 3
    b = np.ascontiguousarray(kinds_b[which])
    e = np.zeros_like(b)
    rows = want_of(kinds_b, np.zeros_like(kinds_b), 4096, 255)
    p, q = np.triu_indices(n_paths)
    cost = np.zeros(len(p), dtype=np.uint64)
    T = table(4096, 255).astype(np.uint64)
    for k in range(3):
        d = rows["deficit"][k].astype(np.int64)
        cost += np.uint64(np.count_nonzero(which == k)) * (np.uint64(4096) * np.minimum(d[p], d[q]).astype(np.uint64) + T[np.abs(d[p] - d[q])])
    assert int(cost.max()) > 1 << 32
    got = ctx.genotype_likelihood_pairs(b, e, 4096, 255)
    assert got["n_scored"] == n_reads and np.array_equal(got["deficit"], rows["deficit"][which])
    bad = np.flatnonzero(got["cost"] != cost)
    assert len(bad) == 0, (len(bad), bad[:4].tolist(), got["cost"][bad[:4]].tolist(), cost[bad[:4]].tolist())


def test_seam_full_table_at_4096_paths(ctx):
    """the whole 8.4 M-pair table against np.triu_indices arithmetic"""
    n_paths = pkg().binding.GENOTYPE_LIK_MAX_PATHS
    b, e = matrices(np.random.default_rng(9), 3, n_paths, 2 * CAP)
    got = ctx.genotype_likelihood_pairs(b, e)
    assert len(got["cost"]) == n_paths * (n_paths + 1) // 2 == 8390656
    ref.same(got, want_of(b, e), "4096 paths")


def test_seam_refuses_bad_arguments(ctx):
    p = pkg()
    L = p.binding.load_library()
    one = np.zeros((1, 1), dtype=np.uint32)
    out = np.zeros(1, dtype=np.uint64)
    u32 = lambda a: p.binding._u32p(a)
    u64 = lambda a: p.binding._u64p(a)
    call = lambda n_reads, n_paths, b, e, lam, cap, c=None: L.vga_genotype_lik_pairs(ctx.h, n_reads, n_paths, b, e, lam, cap, None, c, None)
    assert call(1, 0, u32(one), u32(one), LAM, CAP, u64(out)) == -1
    assert call(1, p.binding.GENOTYPE_LIK_MAX_PATHS + 1, u32(one), u32(one), LAM, CAP) == -1
    assert call(1, 1, None, u32(one), LAM, CAP, u64(out)) == -1
    assert call(1, 1, u32(one), None, LAM, CAP, u64(out)) == -1
    for lam, cap in ((0, CAP), (4097, CAP), (LAM, 0), (LAM, 256)):
        assert call(1, 1, u32(one), u32(one), lam, cap, u64(out)) == -1, (lam, cap)
        with pytest.raises(p.VgaError) as err:
            ctx.genotype_likelihood_pairs(one, one, lam, cap)
        assert err.value.code == -1 and "lambda" in str(err.value)
    with pytest.raises(p.VgaError) as err:
        ctx.genotype_likelihood_pairs(np.zeros((2, 4097), dtype=np.uint32), np.zeros((2, 4097), dtype=np.uint32))
    assert err.value.code == -1 and "4097" in str(err.value)
    # no matrix is needed without reads, and any output may be left out
    assert call(0, 3, None, None, LAM, CAP) == 0
    one[0, 0] = 5
    scored = np.zeros(1, dtype=np.uint64)
    dd = np.full(1, 9, dtype=np.uint8)
    assert L.vga_genotype_lik_pairs(ctx.h, 1, 1, u32(one), u32(one), 4096, 255, dd.ctypes.data_as(p.binding._P(p.binding.C.c_uint8)), None, u64(scored)) == 0
    assert scored[0] == 1 and dd[0] == 0
    assert call(1, 1, u32(one), u32(one), 1, 1, u64(out)) == 0 and out[0] == 0


# =====================================================================================================================
# 2. end to end: the cost table against the reference over the walker's matrices of the oracle's GAF
# =====================================================================================================================
def walker(oracle, ix, seqs, lam=LAM, cap=CAP):
    _, ag, _ = oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, oracle.default_map_params())
    node_len, paths = path_support_ref.parse_gfa(DRB1)
    w = path_support_ref.walk(ag, node_len, paths)
    return want_of(w["bases"], w["edges"], lam, cap), w, ag


def fresh(c, ix, lam=LAM, cap=CAP):
    upload_oracle_index(c, ix)
    g = pkg().hostlib.gfa_paths(DRB1)
    c.path_support_begin(g["step_off"], g["steps"])
    c.genotype_likelihood_begin(lam, cap)


def score(c, seqs, map_params=None):
    b = c.batch(seqs)
    mo = b.map(map_params) if map_params is not None else b.map()
    al = b.align(mo, best_n=1)
    b.close()
    return al, mo


@pytest.fixture(scope="module")
def drb1_case(oracle, drb1):
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)]
    want, w, ag = walker(oracle, drb1, seqs)
    assert w["n_alignments"] == len(seqs) and want["n_paths"] == 12 and want["n_scored"] == len(seqs)
    return seqs, want, w, ag


def test_drb1(ctx, drb1, drb1_case):
    seqs, want, w, _ = drb1_case
    fresh(ctx, drb1)
    score(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_ps_score" in names and all(k in names for k in KERNELS) and "k_gt_pairs" not in names, names
    got = ctx.genotype_likelihood()
    ref.same(got, want, "DRB1 k=11", deficit=False)
    ref.same(ctx.genotype_likelihood(), want, "read twice", deficit=False)
    rank = pkg().binding.genotype_likelihood_rank
    assert rank(got["cost"], 12) == ref.rank(want["cost"], 12) and len(rank(got["cost"], 12)) == 78
    assert rank(got["cost"], 12, 4) == ref.rank(want["cost"], 12, 4)
    # path support itself is what it is without the likelihood
    b, e = ctx.path_support_last()
    assert np.array_equal(b, w["bases"]) and np.array_equal(e, w["edges"])
    assert ctx.path_support()["sum_bases"].tolist() == w["sum_bases"].tolist()
    # the seam over the matrices of the call gives the same table and leaves the context's alone
    ref.same(ctx.genotype_likelihood_pairs(b, e), want, "the seam over the call's matrices")
    ref.same(ctx.genotype_likelihood(), want, "after the seam", deficit=False)
    ctx.path_support_end()


def test_calls_accumulate_and_reset_zeroes(oracle, ctx, drb1, drb1_case):
    seqs, want, _, _ = drb1_case
    s2 = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 7, 1500, 0.03, 0.03, 0.04, seed=52)] + ["ACGT" * 30]
    w2 = walker(oracle, drb1, s2)[0]
    assert w2["n_scored"] == 7  # (the last read has no chain: a placeholder record, a zero row)
    fresh(ctx, drb1)
    score(ctx, seqs)
    score(ctx, s2)
    ref.same(ctx.genotype_likelihood(), ref.add(want, w2), "two different batches", deficit=False)
    ctx.genotype_likelihood_reset()
    got = ctx.genotype_likelihood()
    assert got["n_paths"] == 12 and not got["cost"].any() and got["n_scored"] == 0
    score(ctx, s2)
    ref.same(ctx.genotype_likelihood(), w2, "after reset", deficit=False)
    ctx.path_support_end()


def test_both_strands(oracle, ctx, drb1):
    p = pkg()
    reads = p.readsim.simulate_reads(DRB1, 32, 2500, 0.03, 0.03, 0.04, seed=31, reverse_fraction=0.5)
    seqs = [r.seq for r in reads]
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    fresh(ctx, drb1)
    al, mo = score(ctx, seqs, map_params=mp)
    assert 0 < int(mo.strand.sum()) < len(seqs)
    chosen = [p.readsim.reverse_complement(s) if st else s for s, st in zip(seqs, mo.strand.tolist())]
    ref.same(ctx.genotype_likelihood(), walker(oracle, drb1, chosen)[0], "both strands", deficit=False)
    ctx.path_support_end()


def test_with_coverage_pileup_and_genotype_at_the_same_time(ctx, drb1, drb1_case):
    seqs, want, w, ag = drb1_case
    a = oracle_index_arrays(drb1)
    cov_want = coverage_ref.walk(ag, a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    pile_want = pileup_ref.walk(ag, a["node_seq_idx"], a["seq_fwd"])
    old_want = genotype_ref.pairs(w["bases"], w["edges"])
    fresh(ctx, drb1)
    ctx.genotype_begin()
    ctx.coverage_begin()
    ctx.pileup_begin()
    score(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_cov_add" in names and "k_ps_score" in names and "k_gt_pairs" in names and all(k in names for k in KERNELS), names
    ref.same(ctx.genotype_likelihood(), want, "beside coverage, the pileup and --genotype's table", deficit=False)
    genotype_ref.same(ctx.genotype(), old_want, "--genotype's table is what it is without the likelihood")
    cov = ctx.coverage()
    assert cov[3] == cov_want[3] and all(np.array_equal(g, x) for g, x in zip(cov[:3], cov_want[:3]))
    pile = ctx.pileup()
    assert pile[1] == pile_want[1] and pile[2] == pile_want[2] and np.array_equal(pile[0], pile_want[0])
    assert ctx.path_support()["sum_bases"].tolist() == w["sum_bases"].tolist()
    # the likelihood ends alone and leaves the other four counting
    ctx.genotype_likelihood_end()
    ctx.coverage_reset()
    ctx.pileup_reset()
    ctx.path_support_reset()
    ctx.genotype_reset()
    score(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_ps_score" in names and "k_gt_pairs" in names and not any(k in names for k in KERNELS), names
    genotype_ref.same(ctx.genotype(), old_want, "--genotype goes on")
    assert np.array_equal(ctx.coverage()[0], cov_want[0]) and np.array_equal(ctx.pileup()[0], pile_want[0])
    # and the other way round: --genotype ends, the likelihood goes on
    ctx.genotype_likelihood_begin()
    ctx.genotype_end()
    score(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_gt_pairs" not in names and all(k in names for k in KERNELS), names
    ref.same(ctx.genotype_likelihood(), want, "without --genotype's table", deficit=False)
    ctx.coverage_end()
    ctx.pileup_end()
    ctx.path_support_end()


# =====================================================================================================================
# 3. life cycle
# =====================================================================================================================
def test_life_cycle(drb1, drb1_case):
    p = pkg()
    seqs, _, _, _ = drb1_case
    seqs, n = seqs[:8], 8
    g = p.hostlib.gfa_paths(DRB1)
    c = p.Context(0)
    lik_names = lambda: [t["name"] for t in c.kernel_times() if t["name"].startswith("k_gl")]

    def refused(call, what):
        with pytest.raises(p.VgaError) as e:
            call()
        assert e.value.code == -1, what  # VGA_ERR_ARG

    try:
        refused(c.genotype_likelihood_begin, "begin without an index")
        upload_oracle_index(c, drb1)
        refused(c.genotype_likelihood_begin, "begin without path support")
        assert "path support" in p.binding.load_library().vga_last_error(c.h).decode()
        refused(c.genotype_likelihood, "read before begin")
        refused(c.genotype_likelihood_reset, "reset before begin")
        c.genotype_likelihood_end()  # (ending what is off is harmless)
        c.path_support_begin(g["step_off"], g["steps"])
        refused(c.genotype_likelihood, "path support on, the likelihood off")
        for lam, cap in ((0, CAP), (4097, CAP), (LAM, 0), (LAM, 256)):
            refused(lambda: c.genotype_likelihood_begin(lam, cap), "out of range")
        refused(c.genotype_likelihood, "a refused begin leaves it off")
        score(c, seqs)
        assert lik_names() == [], "off: no launch"
        b, e = c.path_support_last()
        first = want_of(b, e)
        c.genotype_likelihood_begin()
        got = c.genotype_likelihood()
        assert got["n_paths"] == 12 and not got["cost"].any() and got["n_scored"] == 0
        # read checks the size of the table
        L = p.binding.load_library()
        buf = np.zeros(100, dtype=np.uint64)
        assert L.vga_genotype_lik_read(c.h, 77, p.binding._u64p(buf), None) == -1
        assert L.vga_genotype_lik_read(c.h, 78, None, None) == 0
        score(c, seqs)
        assert lik_names() == KERNELS
        ref.same(c.genotype_likelihood(), first, "on", deficit=False)
        assert L.vga_genotype_lik_read(c.h, 78, p.binding._u64p(buf), None) == 0 and np.array_equal(buf[:78], first["cost"])
        # a second begin starts over, with other parameters
        c.genotype_likelihood_begin(100, 255)
        assert not c.genotype_likelihood()["cost"].any()
        score(c, seqs)
        other = want_of(b, e, 100, 255)
        assert not np.array_equal(other["cost"], first["cost"])
        ref.same(c.genotype_likelihood(), other, "lambda 100, cap 255", deficit=False)
        # path_support_end ends it
        c.path_support_end()
        refused(c.genotype_likelihood, "read after path_support_end")
        refused(c.genotype_likelihood_begin, "begin after path_support_end")
        # a second path_support_begin starts path support over, without the likelihood
        c.path_support_begin(g["step_off"], g["steps"])
        c.genotype_likelihood_begin()
        c.path_support_begin(g["step_off"], g["steps"])
        refused(c.genotype_likelihood, "read after a second path_support_begin")
        # a new index ends it
        c.genotype_likelihood_begin()
        upload_oracle_index(c, drb1)
        refused(c.genotype_likelihood, "read after a new index")
        score(c, seqs)
        assert not any(t["name"].startswith(("k_ps", "k_gt", "k_gl")) for t in c.kernel_times())
        # end, then read
        c.path_support_begin(g["step_off"], g["steps"])
        c.genotype_likelihood_begin()
        score(c, seqs)
        ref.same(c.genotype_likelihood(), first, "on again on the new index", deficit=False)
        c.genotype_likelihood_end()
        c.genotype_likelihood_end()
        refused(c.genotype_likelihood, "read after end")
        assert c.path_support()["n_alignments"] == n, "path support goes on"
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
    names = [name for name, _ in paths]
    header = "rank\tpath_a\tpath_b\tcost\tmargin\n"

    def want(top, lam=LAM, cap=CAP, w=w):
        t = want_of(w["bases"], w["edges"], lam, cap)
        ranked = ref.rank(t["cost"], 12, top)
        line = "genotype-likelihood: %s / %s cost %d, next +%d over %d reads" % (names[ranked[0][0]], names[ranked[0][1]], ranked[0][2], ranked[1][3], t["n_scored"])
        return header + "".join("%d\t%s\t%s\t%d\t%d\n" % (i + 1, names[a], names[b], c, m) for i, (a, b, c, m) in enumerate(ranked)), line

    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain")])
    run(common + ["-o", os.path.join(d, "old"), "--genotype", "--genotype-top", "3", "--path-support"])
    L = ["--genotype-likelihood"]
    for out, extra, top, lam, cap in (("one", L, 20, LAM, CAP),
                                      ("two", L + ["--genotype-top", "0", "--devices", "0,0", "--chunk-reads", "10"], 0, LAM, CAP),
                                      ("three", L + ["--genotype-top", "3", "--genotype-lambda", "128", "--genotype-cap", "255", "--genotype", "--path-support",
                                                     "--coverage", "--pileup"], 3, 128, 255)):
        pr = run(common + ["-o", os.path.join(d, out)] + extra)
        pre = os.path.join(d, out)
        tsv, line = want(top, lam, cap)
        assert line in pr.stderr, (line, pr.stderr)
        assert open(pre + "-genotype-likelihood.tsv").read() == tsv, out
        assert open(pre + "-chains.gaf").read() == open(os.path.join(d, "plain-chains.gaf")).read() == ocg, out
        assert open(pre + "-alignments.gaf").read() == open(os.path.join(d, "plain-alignments.gaf")).read() == oag, out
        for other in ("-genotype.tsv", "-path-support.tsv", "-path-support-reads.tsv"):
            assert os.path.exists(pre + other) == (out == "three"), (out, other)
            if out == "three":  # (--genotype's file and path support's are what they are without the likelihood)
                assert open(pre + other).read() == open(os.path.join(d, "old" + other)).read(), other
    assert want(0)[0].count("\n") == 79 and want(20)[0].count("\n") == 21
    assert open(os.path.join(d, "one-genotype-likelihood.tsv")).read() == "".join(open(os.path.join(d, "two-genotype-likelihood.tsv")).readlines()[:21])
    assert not os.path.exists(os.path.join(d, "plain-genotype-likelihood.tsv")) and not os.path.exists(os.path.join(d, "old-genotype-likelihood.tsv"))
    # --both-strands: the GAF files of a run without the switch, and the table of that run's own alignments
    run(common + ["-o", os.path.join(d, "bs"), "--both-strands"])
    pr = run(common + ["-o", os.path.join(d, "four"), "--both-strands"] + L)
    for gaf in ("-chains.gaf", "-alignments.gaf"):
        assert open(os.path.join(d, "four" + gaf)).read() == open(os.path.join(d, "bs" + gaf)).read(), gaf
    tsv, line = want(20, w=path_support_ref.walk(open(os.path.join(d, "bs-alignments.gaf")).read(), node_len, paths))
    assert line in pr.stderr and open(os.path.join(d, "four-genotype-likelihood.tsv")).read() == tsv
    # reads that fit no path: no call, and a table with its header only
    with open(os.path.join(d, "junk.fa"), "w") as f:
        f.write(">j\n%s\n" % ("ACGT" * 30))
    pr = run(common[:4] + [os.path.join(d, "junk.fa")] + common[5:] + ["-o", os.path.join(d, "junk")] + L)
    assert "genotype-likelihood: no call" in pr.stderr, pr.stderr
    assert open(os.path.join(d, "junk-genotype-likelihood.tsv")).read() == header
