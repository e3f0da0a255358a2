"""The set links on the GPU (vga_phase_set_links / vga_phase_set_links_lists: k_ph_obs + k_hc_tags + k_sj_bits + k_sj_pairs;
`vgaligner map --call-variants --phase --phase-join`).  Every comparison is exact equality of the uint32 table with the reference
(tests/phase_join_ref.py): through the kernel seam on synthetic lists (tests/phase_cases.py) at the smallest shapes where the kernels
can go wrong, through a context against the reference run over the oracle's alignments GAF, and through the executable.  Without the
feature every test here stops at Context.phase_set_links_lists / phase_set_links (no such call) or at the unknown --phase-join
flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import haplotag_ref
import haplotype_calls_ref as hc_ref
import phase_cases as P
import phase_join_ref as ref
import phase_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
TILE = 32   # PJ_TILE: the sets on a side of k_sj_pairs' tile of pairs
KERNELS = ("k_ph_obs", "k_hc_tags", "k_sj_bits", "k_sj_pairs")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


def obs_of(case):
    recs, words = P.pack(case.reads)
    return phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref)


def seam(c, case, ps, flip):
    recs, words = P.pack(case.reads)
    return c.phase_set_links_lists(recs, words, case.n_bases, case.pos, case.x, case.y, case.ref, ps, flip)


def same(got, want, what=""):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def launches(c):
    return {t["name"]: t["launches"] for t in c.kernel_times()}


def check(c, case, ps, flip, what):
    want = ref.table(obs_of(case), ps, flip)
    got, n_sets, n_reads = seam(c, case, ps, flip)
    assert n_sets == len(set(ps)) and n_reads == len(case.reads), what
    same(got, want, what)
    return want


def one_set(n):
    return [1] * n


def own_sets(n):
    return [h + 1 for h in range(n)]


def interleaved(n):
    return [1 + (h & 1) for h in range(n)] if n > 1 else [1]


def chained(case):
    ps, flip, _ = phase_ref.chain(phase_ref.tables(obs_of(case), len(case.pos))[0])
    return ps, flip


# ---- 1. the seam
def test_seam_cases_written_out_by_hand(ctx):
    """the tables of tests/test_phase_join_cpu.py: interleaved sets with a flipped site, a tied read, reads without a vote"""
    got, n_sets, n_reads = seam(ctx, P.EDGE, [1, 2, 1, 2, 1], [0, 0, 0, 0, 1])
    assert (n_sets, n_reads) == (2, 6) and got.tolist() == [[4, 0, 0, 1], [3, 1, 0, 0], [3, 0, 0, 1]]
    n = launches(ctx)
    assert all(n.get(k) == 1 for k in KERNELS), n
    assert not any(k in n for k in ("k_ph_link", "k_ph_tag", "k_ph_tag_scan", "k_hc_cols", "k_hc_count")), n
    assert seam(ctx, P.TINY, [1, 2], [0, 0])[0].tolist() == [[2, 0, 0, 1], [1, 1, 0, 1], [1, 0, 0, 3]]
    assert seam(ctx, P.TINY, [1, 1], [0, 1])[0].tolist() == [[2, 0, 0, 0]]
    for ps in ([1, 1, 1, 1, 1], [1, 2, 3, 4, 5], [1, 2, 2, 1, 5], [1, 1, 3, 3, 3]):
        for flip in ([0, 0, 0, 0, 0], [1, 0, 1, 1, 0]):
            check(ctx, P.EDGE, ps, flip, (ps, flip))


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 128, 129])
def test_seam_read_counts(ctx, n_reads):
    """the edges of the ballot word: a partial word, a full one, one read in the second, two full ones, one read in the third; the
    lanes behind the last read count nothing"""
    case = P.random_case("reads", n_reads, 10, seed=700 + n_reads)
    rng = np.random.default_rng(n_reads)
    for name, ps in (("one", one_set(10)), ("own", own_sets(10)), ("interleaved", interleaved(10)), ("chained", chained(case)[0])):
        want = check(ctx, case, ps, [int(v) for v in rng.integers(0, 2, size=10)], "%d reads, %s" % (n_reads, name))
        assert n_reads < 63 or want.sum() > 0


def kinds_case(n_reads, shift):
    """four sites in two interleaved sets (own letter neither allele: a run would show "other"); read r is of kind (r + shift) % 5:
    (a, a), (a, b), (a tie in set 1, b), no vote at all, (b, a)"""
    A, Cc = P.A, P.C
    pos = [2, 5, 8, 11]
    kinds = [([], [(2, A), (5, A)]), ([], [(2, A), (5, Cc)]), ([], [(2, A), (8, Cc), (5, Cc)]), ([], []), ([], [(2, Cc), (8, Cc), (5, A), (11, A)])]
    return P.Case("kinds", 16, pos, [A] * 4, [Cc] * 4, [P.G] * 4, [kinds[(r + shift) % 5] for r in range(n_reads)])


@pytest.mark.parametrize("n_reads", [127, 70])
def test_seam_ties_and_no_votes_in_every_lane(ctx, n_reads):
    """a read tagged on a tie and one without a vote in every lane position of the last, partial word: five shifts of a pattern of
    period five"""
    ps, flip = [1, 2, 1, 2], [0, 0, 0, 0]
    for shift in range(5):
        case = kinds_case(n_reads, shift)
        want = check(ctx, case, ps, flip, (n_reads, shift))
        k = [sum(1 for r in range(n_reads) if (r + shift) % 5 == q) for q in range(5)]
        assert want.tolist() == [[k[0] + k[1], 0, 0, k[4]], [k[0], k[1], k[4], 0], [k[0] + k[4], 0, 0, k[1] + k[2]]], shift


@pytest.mark.parametrize("n_reads", [129, 192])
def test_seam_three_tiles_add_up(ctx, monkeypatch, n_reads):
    """tiles of 64 reads: the sums are carried from tile to tile on the device; the last tile holds one read or is full"""
    case = P.random_case("tiles", n_reads, 12, seed=7 + n_reads)
    reads = list(case.reads)
    for r in (0, 63, 64, 127, n_reads - 1):
        reads[r] = ([(0, case.n_bases)], [])   # a read over every site at the edges of the tiles
    case = case._replace(reads=reads)
    ps, flip = [1, 2, 1, 2, 5, 2, 1, 5, 5, 10, 2, 1], [h % 3 == 1 for h in range(12)]
    want = ref.table(obs_of(case), ps, flip)
    assert want.sum() > 0 and (want[1:4].sum(axis=1) > 0).all()
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    small = seam(ctx, case, ps, flip)[0]
    n = launches(ctx)
    assert all(n.get(k) == 3 for k in KERNELS), n
    same(small, want, "tiles of 64")
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "128")
    two = seam(ctx, case, ps, flip)[0]
    n = launches(ctx)
    assert all(n.get(k) == 2 for k in KERNELS), n
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    whole = seam(ctx, case, ps, flip)[0]
    n = launches(ctx)
    assert all(n.get(k) == 1 for k in KERNELS), n
    assert np.array_equal(small, whole) and np.array_equal(two, whole)


def sets_case(S, seed):
    """2 S sites: the first S open the S sets, the others join sets at random (non-monotone ps; a set that none joins is a set of one
    site); reads that bridge the first, the middle and the last set, so that every tile of pairs counts something"""
    n_sites = 2 * S if S > 1 else 1
    case = P.random_case("sets", 150, n_sites, seed=seed)
    rng = np.random.default_rng(seed)
    ps = own_sets(S) + [int(rng.integers(1, S + 1)) for _ in range(n_sites - S)]
    flip = [int(v) for v in rng.integers(0, 2, size=n_sites)]
    col = lambda a: P.COL_DEL if a == P.D else a
    reads = list(case.reads)
    for s, t in ((0, S - 1), (S // 2, S - 1), (0, S // 2)):
        if s < t:
            for k in range(3):   # twice as x at both, once x and y
                reads.append(([], [(case.pos[s], col(case.x[s])), (case.pos[t], col(case.y[t] if k == 2 else case.x[t]))]))
    return case._replace(reads=reads), ps, flip


@pytest.mark.parametrize("S", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_seam_set_counts(ctx, S):
    """one set, two, a tile of pairs less one, a full one, a second tile with one set, three tiles on a side; a set of one site (the
    opening sites of the sets that no later site joins) and sets whose sites interleave"""
    case, ps, flip = sets_case(S, 800 + S)
    want = check(ctx, case, ps, flip, "%d sets" % S)
    assert len(want) == S * (S + 1) // 2 and len(set(ps)) == S
    if S > 2:
        assert any(ps.count(p) == 1 for p in set(ps)), "a set of one site"
        for s, t in ((0, S - 1), (S // 2, S - 1), (0, S // 2)):
            assert want[ref.pair_index(S, s, t)].sum() >= 3, (s, t)
    # the diagonal: the reads tagged a and b per set, as the rows of vga_phase_tags say on the same input
    recs, words = P.pack(case.reads)
    rows = ctx.phase_tags_lists(recs, words, case.n_bases, case.pos, case.x, case.y, case.ref, ps, flip)
    names = sorted(set(ps))
    for k, p in enumerate(names):
        mine = rows[rows[:, 1] == p]
        d = want[ref.pair_index(S, k, k)].tolist()
        assert d == [int((mine[:, 2] > mine[:, 3]).sum()), 0, 0, int((mine[:, 3] > mine[:, 2]).sum())], p


def raw_lists(c, case, ps, flip, cap_rows, table, n_sets, recs=None, words=None, null=()):
    """vga_phase_set_links_lists itself: the return code; table and n_sets are the caller's"""
    b = pkg().binding
    if recs is None:
        recs, words = P.pack(case.reads)
    rc = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 3)
    wd = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    arrays = {"pos": u32(case.pos), "x": u8(case.x), "y": u8(case.y), "ref": u8(case.ref), "ps": u32(ps), "flip": u8(flip)}
    ptr = lambda k: None if k in null else arrays[k].ctypes.data_as(C.POINTER(C.c_uint32 if arrays[k].dtype == np.uint32 else C.c_uint8))
    pad = lambda a: a if a.size else np.zeros(3, dtype=np.uint32)
    return c.L.vga_phase_set_links_lists(c.h, case.n_bases, len(rc), b._u32p(pad(rc)), len(wd), b._u32p(pad(wd)), len(case.pos), ptr("pos"), ptr("x"), ptr("y"),
                                         ptr("ref"), ptr("ps"), ptr("flip"), cap_rows, None if table is None else b._u32p(table),
                                         None if n_sets is None else C.byref(n_sets))


EDGE_PS, EDGE_FLIP = [1, 2, 1, 2, 5], [0, 0, 0, 0, 1]


def quiet(c):
    """a call that launches nothing: from here on the context reports no kernel, until one is launched"""
    n_sets = C.c_uint64(0)
    assert raw_lists(c, P.EDGE, EDGE_PS, EDGE_FLIP, 0, None, n_sets) == 0 and n_sets.value == 3
    assert not any(k.startswith("k_") for k in launches(c)), launches(c)


def test_seam_cap_below_the_table_counts_nothing(ctx):
    want = ref.table(P.EDGE_OBS, EDGE_PS, EDGE_FLIP)
    assert len(want) == 6
    for cap in (0, 5):
        table, n_sets = np.full((8, 4), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        assert raw_lists(ctx, P.EDGE, EDGE_PS, EDGE_FLIP, cap, table, n_sets) == 0
        assert n_sets.value == 3 and (table == 0xDEADBEEF).all(), cap
        assert not any(k.startswith("k_") for k in launches(ctx)), (cap, launches(ctx))
    n_sets = C.c_uint64(77)
    assert raw_lists(ctx, P.EDGE, EDGE_PS, EDGE_FLIP, 0, None, n_sets) == 0 and n_sets.value == 3     # cap 0 needs no table
    for cap in (6, 8):
        table, n_sets = np.full((8, 4), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        assert raw_lists(ctx, P.EDGE, EDGE_PS, EDGE_FLIP, cap, table, n_sets) == 0 and n_sets.value == 3
        assert table[:6].tolist() == want.tolist() and (table[6:] == 0xDEADBEEF).all(), cap


def test_seam_nothing_to_count(ctx):
    t = P.EDGE
    recs, words = P.pack(t.reads)
    none, n_sets, _ = ctx.phase_set_links_lists(np.zeros((0, 3), dtype=np.uint32), [], t.n_bases, t.pos, t.x, t.y, t.ref, EDGE_PS, EDGE_FLIP)
    assert none.shape == (0, 4) and none.dtype == np.uint32 and n_sets == 0                      # an empty store
    assert not any(k.startswith("k_") for k in launches(ctx))
    none, n_sets, n_reads = ctx.phase_set_links_lists(recs, words, t.n_bases, [], [], [], [], [], [])
    assert none.shape == (0, 4) and n_sets == 0 and n_reads == 6                                   # no site
    got, n_sets, _ = seam(ctx, t._replace(reads=[([(12, 19)], [(15, P.T)])] * 3), EDGE_PS, EDGE_FLIP)   # reads that consume no site
    assert n_sets == 3 and got.shape == (6, 4) and not got.any()


def test_seam_refusals_leave_the_outputs_alone(ctx):
    """everything vga_phase_tags_lists refuses, and more than 4096 sets: nothing launched, table and n_sets untouched, the context
    usable afterwards"""
    t = P.EDGE
    recs, words = P.pack(t.reads)
    want = ref.table(P.EDGE_OBS, EDGE_PS, EDGE_FLIP).tolist()

    def refused(null=(), no_table=False, no_count=False, code=-1, case=None, **changes):
        case = case or t._replace(**{k: v for k, v in changes.items() if k in t._fields})
        table, n_sets = np.full((8, 4), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        quiet(ctx)
        rc = raw_lists(ctx, case, changes.get("ps", EDGE_PS), changes.get("flip", EDGE_FLIP), changes.get("cap", 8), None if no_table else table,
                       None if no_count else n_sets, recs=changes.get("recs", recs), words=changes.get("words", words), null=null)
        assert rc == code, (rc, changes, null)
        assert (table == 0xDEADBEEF).all() and n_sets.value == 77
        assert not any(k.startswith("k_") for k in launches(ctx)), launches(ctx)
        assert seam(ctx, t, EDGE_PS, EDGE_FLIP)[0].tolist() == want

    one = lambda ws, n_runs, n_sparse: dict(recs=[[0, n_runs, n_sparse]], words=ws)
    refused(**one([3 << 1], 1, 0))                         # a run word without its partner
    refused(**one([5 << 1, (3 << 1) | 1], 2, 0))           # end below start
    refused(**one([5 << 1, (41 << 1) | 1], 2, 0))          # end behind the graph
    refused(**one([(40 << 3) | 1], 0, 1))                  # sparse position behind the graph
    refused(**one([(3 << 3) | 7], 0, 1))                   # column 7
    refused(recs=[[2, 0, 1]], words=[0, 0])                # the record starts behind the words
    refused(pos=[0, 10, 11, 39, 20])                       # sites descend
    refused(pos=[0, 10, 11, 20, 40])                       # a site behind the graph
    refused(x=[0, 1, 0, 3, 0])                             # x = y
    refused(y=[1, 4, 2, 3, 5])                             # y above D
    refused(ref=[0, 1, 3, 5, 3])                           # own letter above "other"
    refused(ps=[0, 2, 1, 2, 5])                            # no set 0
    refused(ps=[1, 3, 3, 2, 5])                            # a set named by a later site
    refused(ps=[1, 2, 1, 2, 6])                            # a set named by a site that does not exist
    refused(ps=[1, 1, 2, 2, 5])                            # site 1 does not open a set
    refused(flip=[0, 0, 2, 0, 0])                          # flip above 1
    for k in ("pos", "x", "y", "ref", "ps", "flip"):
        refused(null=(k,))                                 # a NULL array with a non-zero count
    refused(no_table=True)                                 # room for rows and no array
    refused(no_count=True)
    # 4097 singleton sets: refused with the count, before anything is launched; 4096 would be served (its table is not asked for here)
    n = 4097
    many = P.Case("many", 2 * n + 2, [2 * h for h in range(n)], [P.A] * n, [P.C] * n, [P.G] * n, [([(0, 9)], [])])
    quiet(ctx)
    with pytest.raises(pkg().VgaError) as e:
        seam(ctx, many, own_sets(n), [0] * n)
    assert e.value.code == -4 and "4097" in str(e.value), str(e.value)
    assert not any(k.startswith("k_") for k in launches(ctx)), launches(ctx)
    refused(case=many, ps=own_sets(n), flip=[0] * n, recs=[[0, 2, 0]], words=[0, (9 << 1) | 1], code=-4, cap=0)
    n_sets = C.c_uint64(77)
    assert raw_lists(ctx, many._replace(pos=many.pos[:-1], x=many.x[:-1], y=many.y[:-1], ref=many.ref[:-1]), own_sets(n - 1), [0] * (n - 1), 0, None, n_sets) == 0
    assert n_sets.value == 4096 and not any(k.startswith("k_") for k in launches(ctx))


# ---- 2. through a context, and 3. the executable, on one sample
@pytest.fixture(scope="module")
def sample(oracle, drb1):
    """300 reads of 400 bases from the paths of DRB1, the oracle's alignments GAF of them and everything the reference makes of it"""
    reads = pkg().readsim.simulate_reads(DRB1, 300, 400, 0.02, 0.01, 0.01, seed=61)
    a = oracle_index_arrays(drb1)
    _, gaf, _ = oracle.map_reads(drb1, [r.name for r in reads], [r.seq for r in reads])
    g = ref.gaf(gaf, a["node_seq_idx"], a["seq_fwd"])
    assert len(g["obs"]) == len(reads) and g["n_sets"] > 3 and len(g["joins"]) > 0 and g["table"].sum() > 0
    assert g["ps2"] != g["ps"] and ref.check_sets(g["ps2"])
    return dict(g, reads=reads, arrays=a, gaf=gaf)


def test_context_equals_the_reference(ctx, drb1, sample, monkeypatch):
    p = pkg()
    seqs = [r.seq for r in sample["reads"]]
    upload_oracle_index(ctx, drb1)
    ctx.pileup_begin()
    ctx.phase_begin()
    for part in (seqs[:128], seqs[128:]):
        b = ctx.batch(part)
        al = b.align(b.map())
        b.close()
        assert int(al.aligned.sum()) == len(part)
    v = ctx.variant_call()
    het = np.flatnonzero(v["x"] < v["y"])
    pos, x, y = v["pos"][het], v["x"][het], v["y"][het]
    assert pos.tolist() == sample["pos"]
    links, _, n_reads = ctx.phase_links(pos, x, y)
    ps, flip, _ = p.binding.phase_chain(links)
    assert ps.tolist() == sample["ps"] and flip.tolist() == sample["flip"]
    table, n_sets, n = ctx.phase_set_links(pos, x, y, ps, flip)
    assert n == len(seqs) and n_sets == sample["n_sets"]
    n_k = launches(ctx)
    assert all(n_k.get(k) == 1 for k in KERNELS), n_k
    same(table, sample["table"], "the context's store")
    root, sflip, joins, agree, conflict = p.binding.phase_join(table, n_sets)
    assert (root.tolist(), sflip.tolist(), [tuple(j) for j in joins.tolist()], agree, conflict) == \
        (sample["set_root"], sample["set_flip"], sample["joins"], sample["agree"], sample["conflict"])
    # the store is tiled by VGA_PHASE_READ_TILE: 300 reads in five tiles
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    assert np.array_equal(ctx.phase_set_links(pos, x, y, ps, flip)[0], table)
    assert launches(ctx).get("k_sj_pairs") == 5 and launches(ctx).get("k_sj_bits") == 5
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    recs, words = ctx.phase_reads()
    a = sample["arrays"]
    lists = ctx.phase_set_links_lists(recs, words, len(a["seq_fwd"]), pos, x, y, hc_ref.cref_of(a["seq_fwd"], pos), ps, flip)[0]
    assert np.array_equal(lists, table)
    # the joined sets are sets: the tags take them in the place of the chain's
    tags = ctx.phase_tags(pos, x, y, sample["ps2"], sample["flip2"])[0]
    same(tags, haplotag_ref.table(sample["obs"], sample["ps2"], sample["flip2"]), "tags under the joined sets")
    with pytest.raises(p.VgaError) as e:
        ctx.phase_set_links(pos, x, y, np.zeros_like(ps), flip)
    assert e.value.code == -1
    ctx.phase_reset()
    none, n_sets, n = ctx.phase_set_links(pos, x, y, ps, flip)
    assert none.shape == (0, 4) and (n_sets, n) == (0, 0)
    ctx.phase_end()
    with pytest.raises(p.VgaError) as e:
        ctx.phase_set_links(pos, x, y, ps, flip)
    assert e.value.code == -1
    ctx.pileup_end()


def test_cli(drb1, sample, tmp_path):
    d = str(tmp_path)
    a = sample["arrays"]
    fa = os.path.join(d, "r.fa")
    with open(fa, "w") as f:
        for r in sample["reads"]:
            f.write(">%s\n%s\n" % (r.name, r.seq))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1, "--call-variants", "--phase"]
    pr = run(common + ["-o", os.path.join(d, "plain"), "--haplotag", "--haplotype-calls"])
    assert "phase-join" not in pr.stderr and not [f for f in os.listdir(d) if "-phase-jo" in f or "-phase-sets" in f]
    read = lambda name: open(os.path.join(d, name)).read()
    assert read("plain-alignments.gaf") == sample["gaf"]
    new = {"-phase-joined.tsv": sample["joined_tsv"], "-phase-sets.tsv": sample["sets_tsv"], "-phase-joins.tsv": sample["joins_tsv"]}
    # the tags and the haplotype calls of the joined sets
    ids = [i for i, line in enumerate(sample["gaf"].splitlines()) if len(line.split("\t")) >= 12 and line.split("\t")[5] != "*"]
    tag_text = haplotag_ref.tsv(haplotag_ref.rows(sample["obs"], sample["ps2"], sample["flip2"]), ids)[0]
    cpos = [int(q) for q in sample["calls"]["pos"]]
    shows = hc_ref.shows_gaf(sample["gaf"], a["node_seq_idx"], a["seq_fwd"], cpos)
    rows = hc_ref.counts(shows, hc_ref.tags(sample["obs"], sample["ps2"], sample["flip2"]), hc_ref.jobs(cpos, sample["pos"], sample["ps2"]))
    call_text = hc_ref.tsv(rows, cpos, a["node_seq_idx"], a["seq_fwd"])[0]
    assert tag_text != read("plain-haplotag.tsv") and call_text != read("plain-haplotype-calls.tsv")
    for out, extra in (("one", []), ("chunks", ["--chunk-reads", "8"]), ("two", ["--devices", "0,0", "--chunk-reads", "8"])):
        pr = run(common + ["-o", os.path.join(d, out), "--phase-join", "--haplotag", "--haplotype-calls"] + extra)
        for suffix, want in new.items():
            assert read(out + suffix) == want, (out, suffix)
        assert "[vgaligner] " + sample["stderr"] + "\n" in pr.stderr, pr.stderr
        assert read(out + "-haplotag.tsv") == tag_text and read(out + "-haplotype-calls.tsv") == call_text, out
        # every other file is byte for byte what it is without the switch
        files = {f[len(out):] for f in os.listdir(d) if f.startswith(out + "-")}
        assert files == {f[len("plain"):] for f in os.listdir(d) if f.startswith("plain-")} | set(new)
        for suffix in files - set(new) - {"-haplotag.tsv", "-haplotype-calls.tsv"}:
            assert read(out + suffix) == read("plain" + suffix), (out, suffix)
        assert "-phase.tsv" in files and "-variants.tsv" in files
    # the switch alone, and another --phase-join-min-reads
    strict = ref.gaf(sample["gaf"], a["node_seq_idx"], a["seq_fwd"], min_reads=4)
    assert strict["joins"] != sample["joins"]
    pr = run(common + ["-o", os.path.join(d, "strict"), "--phase-join", "--phase-join-min-reads", "4"])
    assert read("strict-phase-joins.tsv") == strict["joins_tsv"] and read("strict-phase-sets.tsv") == strict["sets_tsv"]
    assert read("strict-phase-joined.tsv") == strict["joined_tsv"] and strict["stderr"] in pr.stderr
    assert read("strict-phase.tsv") == read("plain-phase.tsv") and not os.path.exists(os.path.join(d, "strict-haplotag.tsv"))
    # no heterozygous site: the headers only
    pr = run(common + ["-o", os.path.join(d, "none"), "--phase-join", "--call-min-depth", "1000"])
    assert read("none-phase-sets.tsv") == ref.SETS_HEADER + "\n" and read("none-phase-joins.tsv") == ref.JOINS_HEADER + "\n"
    assert read("none-phase-joined.tsv") == phase_ref.HEADER + "\n" and ref.stderr_line(0, [], 0, 0) in pr.stderr
