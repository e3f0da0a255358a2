"""The haplotype tags on the GPU (vga_phase_tags / vga_phase_tags_lists, k_ph_obs + k_ph_tag + k_ph_tag_scan, `vgaligner map
--call-variants --phase --haplotag`).  Every comparison is exact equality of the uint32 rows with the reference
(tests/haplotag_ref.py): through the kernel seam on synthetic lists (tests/phase_cases.py) at the smallest shapes where the kernels
can go wrong, through a context against the reference run over the oracle's alignments GAF, and through the executable.  Without
the feature every test here stops at Context.phase_tags_lists / phase_tags (no such call) or at the unknown --haplotag flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import haplotag_ref
import phase_cases as P
import phase_ref
import variant_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


def observations(case):
    recs, words = P.pack(case.reads)
    return phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref)


def seam(c, case, ps, flip, **kw):
    recs, words = P.pack(case.reads)
    return c.phase_tags_lists(recs, words, case.n_bases, case.pos, case.x, case.y, case.ref, ps, flip, **kw)


def same(got, want, what=""):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


# the ways to group H sites: (name, ps)
def one_set(H):
    return [1] * H


def own_sets(H):
    return [h + 1 for h in range(H)]


def interleaved(H):
    """even sites in set 1, odd sites in set 2: ps is not monotone in h"""
    return [1 + (h & 1) for h in range(H)]


def chained(case):
    """the sets and flips the chain gives on the case's own links"""
    ps, flip, _ = phase_ref.chain(phase_ref.tables(observations(case), len(case.pos))[0])
    return ps, flip


def check(c, case, ps, flip, what):
    want = haplotag_ref.table(observations(case), ps, flip)
    same(seam(c, case, ps, flip), want, what)
    return want


# ---- 1. the seam
def test_seam_cases_written_out_by_hand(ctx):
    """the rows of test_haplotag_cpu.py: a flipped site, ties, reads without a row, interleaved sets"""
    got = seam(ctx, P.TINY, [1, 1], [0, 1])
    assert got.tolist() == [[0, 1, 2, 0], [1, 1, 1, 1], [2, 1, 1, 1], [3, 1, 1, 0]]
    launches = {t["name"]: t["launches"] for t in ctx.kernel_times()}
    assert launches.get("k_ph_obs") == 1 and launches.get("k_ph_tag") == 2 and launches.get("k_ph_tag_scan") == 1 and "k_ph_link" not in launches, launches
    assert seam(ctx, P.TINY, [1, 2], [0, 0]).tolist() == [[0, 1, 1, 0], [0, 2, 0, 1], [1, 1, 0, 1], [1, 2, 0, 1], [2, 1, 1, 0], [2, 2, 1, 0], [3, 2, 0, 1]]
    got = seam(ctx, P.EDGE, [1, 2, 1, 2, 1], [0, 1, 1, 0, 1])
    assert got.tolist() == [[0, 1, 2, 0], [0, 2, 0, 1], [1, 1, 1, 0], [1, 2, 1, 0], [2, 1, 0, 1], [2, 2, 0, 1], [3, 1, 1, 0], [3, 2, 0, 2], [5, 1, 2, 0], [5, 2, 1, 0]]
    same(got, haplotag_ref.table(P.EDGE_OBS, [1, 2, 1, 2, 1], [0, 1, 1, 0, 1]), "edge")
    far = P.far_case()
    for ps in (one_set(10), own_sets(10), chained(far)[0]):
        assert len(check(ctx, far, ps, [0, 1] * 5, "far")) > 0


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 129])
def test_seam_read_counts(ctx, n_reads):
    """a partial wave, a full one, a second workgroup; the lanes behind the last read write nothing"""
    case = P.random_case("reads", n_reads, 10, seed=200 + n_reads)
    rng = np.random.default_rng(n_reads)
    for name, ps in (("one", one_set(10)), ("own", own_sets(10)), ("interleaved", interleaved(10)), ("chained", chained(case)[0])):
        flip = [int(v) for v in rng.integers(0, 2, size=10)]
        want = check(ctx, case, ps, flip, "%d reads, %s" % (n_reads, name))
        assert n_reads == 1 or len(want) > 0


@pytest.mark.parametrize("n_sites", [1, 8, 9, 65])
def test_seam_site_counts(ctx, n_sites):
    """sets shorter and longer than the unrolled part of the site loop, more sites than a wave has lanes"""
    case = P.random_case("sites", 70, n_sites, seed=300 + n_sites)
    rng = np.random.default_rng(n_sites)
    ps_chain, flip_chain = chained(case)
    for name, ps, flip in (("one", one_set(n_sites), None), ("own", own_sets(n_sites), None), ("interleaved", interleaved(n_sites), None),
                           ("chained", ps_chain, flip_chain)):
        flip = flip if flip is not None else [int(v) for v in rng.integers(0, 2, size=n_sites)]
        want = check(ctx, case, ps, flip, "%d sites, %s" % (n_sites, name))
        assert len(want) > 0
    # three sets of unequal size whose opening sites are 0, 1 and 5
    if n_sites >= 9:
        ps = [1, 2, 1, 1, 2, 6, 6, 1, 6] + [1] * (n_sites - 9)
        check(ctx, case, ps, [h % 3 == 0 for h in range(n_sites)], "three sets")


def tiles_case():
    """129 reads for tiles of 64: the first and the last read of the first two tiles consume no site (no rows), the one read of
    the third tile and the neighbours of the empty ones span every site (rows)"""
    case = P.random_case("tiles", 129, 12, seed=7)
    reads = list(case.reads)
    for r in (0, 63, 64, 127):
        reads[r] = ([], [])
    for r in (1, 62, 65, 126, 128):
        reads[r] = ([(0, case.n_bases)], [])
    return case._replace(reads=reads)


def test_seam_three_tiles_offsets_carried(ctx, monkeypatch):
    case = tiles_case()
    ps, flip = interleaved(12), [h % 3 == 1 for h in range(12)]
    want = haplotag_ref.table(observations(case), ps, flip)
    with_rows = set(want[:, 0].tolist())
    assert not with_rows & {0, 63, 64, 127} and {1, 62, 65, 126, 128} <= with_rows and len(want) > 129
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    small = seam(ctx, case, ps, flip)
    launches = {t["name"]: t["launches"] for t in ctx.kernel_times()}
    assert launches.get("k_ph_obs") == 3 and launches.get("k_ph_tag") == 6 and launches.get("k_ph_tag_scan") == 3, launches
    same(small, want, "tiles of 64")
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "128")
    two = seam(ctx, case, ps, flip)
    assert {t["name"]: t["launches"] for t in ctx.kernel_times()}.get("k_ph_obs") == 2
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    whole = seam(ctx, case, ps, flip)
    assert {t["name"]: t["launches"] for t in ctx.kernel_times()}.get("k_ph_obs") == 1
    assert np.array_equal(small, whole) and np.array_equal(two, whole)
    # the ask-again protocol across tiles: a first answer without room for a row
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    same(seam(ctx, case, ps, flip, cap=0), want, "tiles of 64, asked again")


def raw_lists(c, case, ps, flip, cap, rows, n_rows, recs=None, words=None, null=()):
    """vga_phase_tags_lists itself: the return code; rows and n_rows are the caller's"""
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
    return c.L.vga_phase_tags_lists(c.h, case.n_bases, len(rc), b._u32p(pad(rc)), len(wd), b._u32p(pad(wd)), len(case.pos), ptr("pos"), ptr("x"), ptr("y"),
                                    ptr("ref"), ptr("ps"), ptr("flip"), cap, None if rows is None else b._u32p(rows), None if n_rows is None else C.byref(n_rows))


def test_seam_cap_cuts_the_rows_not_the_count(ctx):
    case = P.random_case("cap", 65, 9, seed=11)
    ps, flip = interleaved(9), [0, 1, 0, 0, 1, 1, 0, 1, 0]
    want = haplotag_ref.table(observations(case), ps, flip)
    n = len(want)
    assert n > 65
    for cap in (0, 1, n - 1, n, n + 5):
        rows, n_rows = np.full((n + 8, 4), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        assert raw_lists(ctx, case, ps, flip, cap, rows, n_rows) == 0
        assert n_rows.value == n, cap
        assert np.array_equal(rows[:min(cap, n)], want[:min(cap, n)]) and (rows[min(cap, n):] == 0xDEADBEEF).all(), cap
    n_rows = C.c_uint64(77)
    assert raw_lists(ctx, case, ps, flip, 0, None, n_rows) == 0 and n_rows.value == n     # cap 0 needs no rows array
    same(seam(ctx, case, ps, flip, cap=0), want, "asked again from 0")
    same(seam(ctx, case, ps, flip, cap=n - 1), want, "asked again from n - 1")


def test_seam_nothing_to_tag(ctx):
    none = ctx.phase_tags_lists(np.zeros((0, 3), dtype=np.uint32), [], 20, [3, 7], [0, 1], [2, 3], [0, 3], [1, 1], [0, 0])
    assert none.shape == (0, 4) and none.dtype == np.uint32
    recs, words = P.pack(P.TINY.reads)
    assert ctx.phase_tags_lists(recs, words, 20, [], [], [], [], [], []).shape == (0, 4)
    # reads that consume no site
    assert ctx.phase_tags_lists([[0, 0, 0], [0, 2, 0]], [8 << 1, (12 << 1) | 1], 20, [3, 7], [0, 1], [2, 3], [0, 3], [1, 1], [0, 0]).shape == (0, 4)


def test_a_call_that_launches_nothing_reports_no_kernel(drb1):
    """links, tags and counts, from lists and from the store, without sites and without reads: kernel_times() holds the kernels of the
    last call, so none -- not those of the call that launched before it"""
    p = pkg()
    sites = ([3, 7], [0, 1], [2, 3])
    lists = ([[0, 2, 0]], [0 << 1, (10 << 1) | 1], 20)
    no_reads, no_sites = (np.zeros((0, 3), dtype=np.uint32), [], 20), ([], [], [])
    c = p.Context(0)
    try:
        upload_oracle_index(c, drb1)
        c.pileup_begin()
        c.phase_begin()
        c.phase_reset()
        quiet = [lambda: c.phase_links_lists(*lists, *no_sites, []), lambda: c.phase_links_lists(*no_reads, *sites, [0, 3]),
                 lambda: c.phase_tags_lists(*lists, *no_sites, [], [], []), lambda: c.phase_tags_lists(*no_reads, *sites, [0, 3], [1, 1], [0, 0]),
                 lambda: c.haplotype_counts_lists(*lists, [5], [0], *no_sites, [], [], []),
                 lambda: c.haplotype_counts_lists(*no_reads, [5], [0], *sites, [0, 3], [1, 1], [0, 0]),
                 lambda: c.phase_links(*no_sites), lambda: c.phase_links(*sites),
                 lambda: c.phase_tags(*no_sites, [], []), lambda: c.phase_tags(*sites, [1, 1], [0, 0]),
                 lambda: c.haplotype_counts([5], *no_sites, [], []), lambda: c.haplotype_counts([5], *sites, [1, 1], [0, 0])]
        for k, call in enumerate(quiet):
            links, sr = c.phase_links_lists(*lists, *sites, [0, 3])   # one read over both sites: it launches
            assert sr.tolist() == [[1, 0, 0], [0, 1, 0]] and {"k_ph_obs", "k_ph_link"} <= {t["name"] for t in c.kernel_times()}
            call()
            assert not [t["name"] for t in c.kernel_times() if t["name"].startswith("k_")], (k, c.kernel_times())
    finally:
        c.close()


def test_seam_refusals_leave_the_outputs_alone(ctx):
    """everything vga_phase_links_lists refuses and what the sets add: VGA_ERR_ARG, nothing launched, rows and n_rows untouched,
    the context usable afterwards"""
    t = P.TINY
    recs, words = P.pack(t.reads)

    def refused(ps=(1, 1), flip=(0, 1), null=(), no_rows=False, no_count=False, **changes):
        case = t._replace(**{k: v for k, v in changes.items() if k in t._fields})
        rows, n_rows = np.full((16, 4), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        rc = raw_lists(ctx, case, list(ps), list(flip), 16, None if no_rows else rows, None if no_count else n_rows, recs=changes.get("recs", recs),
                       words=changes.get("words", words), null=null)
        assert rc == -1, (rc, changes, ps, flip, null)
        assert (rows == 0xDEADBEEF).all() and n_rows.value == 77
        assert seam(ctx, t, [1, 1], [0, 1]).tolist() == [[0, 1, 2, 0], [1, 1, 1, 1], [2, 1, 1, 1], [3, 1, 1, 0]]

    one = lambda ws, n_runs, n_sparse: dict(recs=[[0, n_runs, n_sparse]], words=ws)
    refused(**one([3 << 1], 1, 0))                         # a run word without its partner
    refused(**one([5 << 1, (3 << 1) | 1], 2, 0))           # end below start
    refused(**one([5 << 1, (21 << 1) | 1], 2, 0))          # end behind the graph
    refused(**one([(20 << 3) | 1], 0, 1))                  # sparse position behind the graph
    refused(**one([(3 << 3) | 7], 0, 1))                   # column 7
    refused(recs=[[2, 0, 1]], words=[0, 0])                # the record starts behind the words
    refused(pos=[7, 3])                                    # sites descend
    refused(pos=[3, 20])                                   # a site behind the graph
    refused(x=[2, 1])                                      # x = y
    refused(y=[2, 5])                                      # y above D
    refused(ref=[0, 5])                                    # own letter above "other"
    refused(ps=[0, 1])                                     # no set 0
    refused(ps=[2, 2])                                     # a set named by a later site
    refused(ps=[1, 3])                                     # a set named by a site that does not exist
    refused(flip=[0, 2])                                   # flip above 1
    three = dict(pos=[3, 7, 9], x=[0, 1, 0], y=[2, 3, 1], ref=[0, 3, 0], flip=[0, 0, 0])
    refused(ps=[1, 1, 2], **three)                         # site 1 does not open a set: it is in set 1
    for k in ("pos", "x", "y", "ref", "ps", "flip"):
        refused(null=(k,))                                 # a NULL array with sites
    refused(no_rows=True)                                  # room for rows and no array
    refused(no_count=True)
    rows, n_rows = np.full((16, 4), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
    assert raw_lists(ctx, t._replace(**{k: v for k, v in three.items() if k in t._fields}), [1, 1, 3], three["flip"], 16, rows, n_rows) == 0   # (and that one is fine)


# ---- 2. through a context, and 3. the executable, on one sample
@pytest.fixture(scope="module")
def sample(oracle, drb1):
    """300 reads of 400 bases from the paths of DRB1, the oracle's alignments GAF of them and the reference's sites, chain and rows"""
    reads = pkg().readsim.simulate_reads(DRB1, 300, 400, 0.02, 0.01, 0.01, seed=61)
    a = oracle_index_arrays(drb1)
    _, gaf, _ = oracle.map_reads(drb1, [r.name for r in reads], [r.seq for r in reads])
    calls = variant_ref.call_gaf(gaf, a["node_seq_idx"], a["seq_fwd"])
    pos, x, y = phase_ref.sites_of(calls)
    obs = phase_ref.observations(gaf, a["node_seq_idx"], a["seq_fwd"], pos, x, y)
    ps, flip, _ = phase_ref.chain(phase_ref.tables(obs, len(pos))[0])
    rows = haplotag_ref.table(obs, ps, flip)
    assert len(obs) == len(reads) and len(rows) > 300 and len(set(ps)) > 10 and any(flip)
    assert any(haplotag_ref.hap(int(r[2]), int(r[3])) == "." for r in rows)
    return {"reads": reads, "arrays": a, "gaf": gaf, "pos": pos, "x": x, "y": y, "ps": ps, "flip": flip, "rows": rows}


def test_context_equals_the_reference(ctx, drb1, sample, monkeypatch):
    """map, align with the store on, call, link, chain, tag: the rows of the context's own store are those of the reference on
    the oracle's GAF, those of its store fed through the seam, and the same under a tile of 64 reads"""
    p = pkg()
    a = sample["arrays"]
    seqs = [r.seq for r in sample["reads"]]
    upload_oracle_index(ctx, drb1)
    ctx.pileup_begin()
    ctx.phase_begin()
    for part in (seqs[:128], seqs[128:]):      # two align calls: the records of the second follow those of the first
        b = ctx.batch(part)
        al = b.align(b.map())
        b.close()
        assert int(al.aligned.sum()) == len(part)
    v = ctx.variant_call()
    het = np.flatnonzero(v["x"] < v["y"])
    pos, x, y = v["pos"][het], v["x"][het], v["y"][het]
    assert pos.tolist() == sample["pos"] and x.tolist() == sample["x"] and y.tolist() == sample["y"]
    links, _, n_reads = ctx.phase_links(pos, x, y)
    ps, flip, _ = p.binding.phase_chain(links)
    assert n_reads == len(seqs) and ps.tolist() == sample["ps"] and flip.tolist() == sample["flip"]
    rows, n = ctx.phase_tags(pos, x, y, ps, flip)
    assert n == len(seqs)
    launches = {t["name"]: t["launches"] for t in ctx.kernel_times()}
    assert launches.get("k_ph_tag") == 2 * launches.get("k_ph_obs") and launches.get("k_ph_tag_scan") == launches.get("k_ph_obs"), launches
    same(rows, sample["rows"], "the context's store")
    same(ctx.phase_tags(pos, x, y, ps, flip, cap=1)[0], sample["rows"], "asked again")
    recs, words = ctx.phase_reads()
    ref = [min(4, phase_ref.allele(chr(a["seq_fwd"][int(q)]))) for q in pos]
    lists = ctx.phase_tags_lists(recs, words, len(a["seq_fwd"]), pos, x, y, ref, ps, flip)
    assert np.array_equal(lists, rows)
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    assert np.array_equal(ctx.phase_tags(pos, x, y, ps, flip)[0], rows)
    assert {t["name"]: t["launches"] for t in ctx.kernel_times()}.get("k_ph_obs") == 5
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    # the calls refuse what the seam refuses, and the store is needed
    for bad in (dict(ps=np.zeros_like(ps)), dict(flip=np.full_like(flip, 2))):
        with pytest.raises(p.VgaError) as e:
            ctx.phase_tags(pos, x, y, bad.get("ps", ps), bad.get("flip", flip))
        assert e.value.code == -1
    ctx.phase_reset()
    assert ctx.phase_tags(pos, x, y, ps, flip)[0].shape == (0, 4)
    ctx.phase_end()
    with pytest.raises(p.VgaError) as e:
        ctx.phase_tags(pos, x, y, ps, flip)
    assert e.value.code == -1
    b = ctx.batch(seqs[:8])
    b.align(b.map())
    b.close()
    assert not any(t["name"].startswith("k_ph") for t in ctx.kernel_times()), "store off: no phase kernel"
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
    pr = run(common + ["-o", os.path.join(d, "plain")])
    assert not os.path.exists(os.path.join(d, "plain-haplotag.tsv")) and "haplotag" not in pr.stderr
    read = lambda name: open(os.path.join(d, name)).read()
    assert read("plain-alignments.gaf") == sample["gaf"]
    want, n_rows, n_a, n_b, n_tied, n_records = haplotag_ref.tsv_gaf(sample["gaf"], a["node_seq_idx"], a["seq_fwd"])
    assert want == haplotag_ref.tsv(sample["rows"])[0] and n_rows == len(sample["rows"]) and n_tied > 0
    for out, extra in (("one", []), ("chunks", ["--chunk-reads", "10"]), ("two", ["--devices", "0,0", "--chunk-reads", "10"])):
        pr = run(common + ["-o", os.path.join(d, out), "--haplotag"] + extra)
        assert read(out + "-haplotag.tsv") == want, out
        assert "haplotag: %d rows of %d reads: %d a, %d b, %d undecided" % (n_rows, n_records, n_a, n_b, n_tied) in pr.stderr, pr.stderr
        # every other file is byte for byte what it is without the switch
        files = {f[len(out):] for f in os.listdir(d) if f.startswith(out + "-")}
        assert files == {f[len("plain"):] for f in os.listdir(d) if f.startswith("plain-")} | {"-haplotag.tsv"}
        for suffix in files - {"-haplotag.tsv"}:
            assert read(out + suffix) == read("plain" + suffix), (out, suffix)
    # no heterozygous site: the header only
    pr = run(common + ["-o", os.path.join(d, "none"), "--haplotag", "--call-min-depth", "1000"])
    assert read("none-haplotag.tsv") == haplotag_ref.HEADER + "\n" and "haplotag: 0 rows of %d reads: 0 a, 0 b, 0 undecided" % len(sample["reads"]) in pr.stderr
    # reads that are not aligned keep their number: the file numbers the reads of the input
    with open(fa, "w") as f:
        for i, r in enumerate(sample["reads"][:120]):
            f.write(">%s\n%s\n" % (r.name, "ACGT" * 30 if i in (0, 17, 64) else r.seq))
    pr = run(common + ["-o", os.path.join(d, "gaps"), "--haplotag", "--devices", "0,0", "--chunk-reads", "9"])
    want, n_rows, n_a, n_b, n_tied, n_records = haplotag_ref.tsv_gaf(read("gaps-alignments.gaf"), a["node_seq_idx"], a["seq_fwd"])
    assert n_records == 117 and n_rows > 100 and read("gaps-haplotag.tsv") == want
    assert "haplotag: %d rows of 117 reads" % n_rows in pr.stderr, pr.stderr
    pr = subprocess.run([EXE, "map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1, "--call-variants", "--haplotag", "-o",
                         os.path.join(d, "bad")], cwd=d, capture_output=True, text=True, timeout=300)
    assert pr.returncode != 0 and "--phase" in pr.stderr and not [f for f in os.listdir(d) if f.startswith("bad")]
