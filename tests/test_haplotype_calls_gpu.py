"""The haplotype counts on the GPU (vga_haplotype_counts / vga_haplotype_counts_lists: k_ph_obs + k_hc_tags + k_hc_cols + k_hc_count;
`vgaligner map --call-variants --phase --haplotag --haplotype-calls`).  Every comparison is exact equality of the uint32 rows with
the reference (tests/haplotype_calls_ref.py): through the kernel seam on synthetic lists (tests/hapcall_cases.py, tests/phase_cases.py)
at the smallest shapes where the kernels can go wrong, through a context against the reference run over the oracle's alignments
GAF, and through the executable.  Without the feature every test here stops at Context.haplotype_counts_lists / haplotype_counts
(no such call) or at the unknown --haplotype-calls flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hapcall_cases as H
import haplotag_ref
import haplotype_calls_ref as ref
import phase_cases as P
import phase_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
COUNT_BLOCK = 256   # HC_COUNT_BLOCK: the reads one pass of k_hc_count's workgroup takes


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


def want_rows(case):
    recs, words = P.pack(case.reads)
    obs = phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref)
    return ref.table(ref.shows_lists(recs, words, case.cpos, case.cref), obs, case.cpos, case.pos, case.ps, case.flip)


def seam(c, case, **kw):
    recs, words = P.pack(case.reads)
    return c.haplotype_counts_lists(recs, words, case.n_bases, case.cpos, case.cref, case.pos, case.x, case.y, case.ref, case.ps, case.flip, **kw)


def same(got, want, what=""):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def launches(c):
    return {t["name"]: t["launches"] for t in c.kernel_times()}


def one_set(n):
    return [1] * n


def own_sets(n):
    return [h + 1 for h in range(n)]


def interleaved(n):
    return [1 + (h & 1) for h in range(n)]


def nested(n):
    """set 1 holds the first and the last site, set 2 everything between them"""
    return [1] + [2] * (n - 2) + [1] if n >= 3 else [1] * n


def chained(case):
    recs, words = P.pack(case.reads)
    ps, flip, _ = phase_ref.chain(phase_ref.tables(phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref), len(case.pos))[0])
    return ps, flip


def check(c, case, what):
    want = want_rows(case)
    same(seam(c, case), want, what)
    return want


# ---- 1. the seam
def test_seam_cases_written_out_by_hand(ctx):
    """interleaved sets with a flipped site; calls before the first site, behind the last and in one set alone; a tied read and reads
    without a row that count nowhere; two sparse words on one base, a run plus a sparse word, an insertion word twice, a call whose own
    letter is no A C G T under a run; every column shown by a read tagged a, by one tagged b, by a tied one and by one without a row"""
    got = seam(ctx, H.HAND)
    assert got.tolist() == H.HAND_ROWS and len(got) == 10
    n = launches(ctx)
    assert n.get("k_ph_obs") == 1 and n.get("k_hc_tags") == 1 and n.get("k_hc_cols") == 1 and n.get("k_hc_count") == 1, n
    assert not any(k in n for k in ("k_ph_link", "k_ph_tag", "k_ph_tag_scan")), n
    for copies in (1, 3):
        case, rows = H.columns_case(copies)
        assert seam(ctx, case).tolist() == rows, copies
    # the other groupings of the same four sites: own-site sets (J = 4), nested (J = 10), behind each other (J = 6, base 15 between them)
    for ps, n_jobs in (([1, 2, 3, 4], 4), ([1, 2, 2, 1], 10), ([1, 1, 3, 3], 6)):
        for flip in ([0, 0, 0, 0], [1, 0, 1, 1]):
            want = check(ctx, H.HAND._replace(ps=ps, flip=flip), (ps, flip))
            assert len(want) == n_jobs
    # an insertion word at a base the read does not consume, and nothing else at the call
    case = H.HAND._replace(reads=[([(0, 10)], [(15, H.COL_INS)]), ([], [(5, H.C), (20, H.A), (15, H.COL_INS)])], ps=[1, 1, 1, 1], flip=[0, 0, 0, 0])
    got = seam(ctx, case)
    same(got, want_rows(case), "insertion alone")
    assert got[3].tolist() == [4, 1] + [0] * 6 + [1] + [0] * 7   # read 0 is a (site 0 alone), read 1 is tied: no b


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 129, COUNT_BLOCK + 1])
def test_seam_read_counts(ctx, n_reads):
    """a partial wave, a full one, a second wave of k_hc_count, a second pass of its workgroup; the lanes behind the last read count
    nothing"""
    case = P.random_case("reads", n_reads, 10, seed=400 + n_reads)
    rng = np.random.default_rng(n_reads)
    for name, ps in (("one", one_set(10)), ("own", own_sets(10)), ("interleaved", interleaved(10)), ("nested", nested(10)), ("chained", chained(case)[0])):
        h = H.with_calls(case, 12, ps, rng.integers(0, 2, size=10), seed=n_reads)
        want = check(ctx, h, "%d reads, %s" % (n_reads, name))
        assert len(want) > 0 and (n_reads < 63 or want[:, 2:].sum() > 0)


@pytest.mark.parametrize("n_sites", [1, 8, 9, 65])
def test_seam_site_counts(ctx, n_sites):
    case = P.random_case("sites", 70, n_sites, seed=500 + n_sites)
    rng = np.random.default_rng(n_sites)
    ps_chain, flip_chain = chained(case)
    for name, ps, flip in (("one", one_set(n_sites), None), ("own", own_sets(n_sites), None), ("interleaved", interleaved(n_sites), None),
                           ("nested", nested(n_sites), None), ("chained", ps_chain, flip_chain)):
        flip = flip if flip is not None else rng.integers(0, 2, size=n_sites)
        h = H.with_calls(case, min(case.n_bases, 2 * n_sites + 3), ps, flip, seed=n_sites)
        want = check(ctx, h, "%d sites, %s" % (n_sites, name))
        assert len(want) > 0 and want[:, 2:].sum() > 0


@pytest.mark.parametrize("n_calls", [1, 3, 4, 5, 65])
def test_seam_call_counts(ctx, n_calls):
    """fewer calls than a word of the byte rows holds, one more, more than a wave has lanes"""
    case = P.random_case("calls", 70, 9, seed=600 + n_calls, n_bases=90)
    rng = np.random.default_rng(n_calls)
    for name, ps in (("one", one_set(9)), ("own", own_sets(9)), ("interleaved", interleaved(9)), ("three", [1, 2, 1, 1, 2, 6, 6, 1, 6])):
        h = H.with_calls(case, n_calls, ps, rng.integers(0, 2, size=9), seed=n_calls)
        want = check(ctx, h, "%d calls, %s" % (n_calls, name))
        assert len(want) == len(ref.jobs(h.cpos, h.pos, h.ps))
    if n_calls == 1:   # the one call on a site, every site its own set: the one job of that set
        h = H.with_calls(case, 1, own_sets(9), [0] * 9, seed=1)._replace(cpos=[case.pos[4]], cref=[case.ref[4]])
        assert check(ctx, h, "own site")[:, :2].tolist() == [[0, 5]]


def tiles_case():
    case = P.random_case("tiles", 129, 12, seed=7)
    reads = list(case.reads)
    for r in (0, 63, 64, 127):
        reads[r] = ([], [])
    for r in (1, 62, 65, 126, 128):
        reads[r] = ([(0, case.n_bases)], [])
    ps, flip = interleaved(12), [h % 3 == 1 for h in range(12)]
    return H.with_calls(case._replace(reads=reads), 20, ps, flip, seed=3)


def test_seam_three_tiles_add_up(ctx, monkeypatch):
    case = tiles_case()
    want = want_rows(case)
    assert len(want) > 20 and want[:, 2:].sum() > 0
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    small = seam(ctx, case)
    n = launches(ctx)
    assert n.get("k_ph_obs") == 3 and n.get("k_hc_tags") == 3 and n.get("k_hc_cols") == 3 and n.get("k_hc_count") == 3, n
    same(small, want, "tiles of 64")
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "128")
    two = seam(ctx, case)
    n = launches(ctx)
    assert n.get("k_ph_obs") == 2 and n.get("k_hc_tags") == 2 and n.get("k_hc_cols") == 2 and n.get("k_hc_count") == 2, n
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    whole = seam(ctx, case)
    n = launches(ctx)
    assert n.get("k_ph_obs") == 1 and n.get("k_hc_tags") == 1 and n.get("k_hc_cols") == 1 and n.get("k_hc_count") == 1, n
    assert np.array_equal(small, whole) and np.array_equal(two, whole)
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    same(seam(ctx, case, cap=0), want, "tiles of 64, asked again")


def test_seam_links_tags_and_counts_in_any_order(ctx, monkeypatch):
    """the three calls that share the frame of a tile (the reads, the sites, the tile behind k_ph_obs) on one case and one context,
    each of them first, in the middle and last: 129 reads in tiles of 64, 64 and 1, nine sites (the window of eight and one more), the
    sets of the chain on the case's own links.  Every result equals its reference, so it is the same whatever ran before it."""
    case = P.random_case("frame", 129, 9, seed=23)
    recs, words = P.pack(case.reads)
    obs = phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref)
    links, site_reads = phase_ref.tables(obs, 9)
    ps, flip, _ = pkg().binding.phase_chain(links)
    h = H.with_calls(case, 20, ps, flip, seed=23)
    tags, rows = haplotag_ref.table(obs, ps, flip), want_rows(h)
    # four sets, one of them inside the span of another, a flipped site; the one read of the last tile has tag rows
    assert ps.tolist() == [1, 2, 3, 2, 2, 2, 7, 2, 2] and flip.any() and tags[-1, 0] == 128 and len(rows) > 9 and rows[:, 2:].sum() > 0
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    sites = (case.n_bases, case.pos, case.x, case.y, case.ref)

    def run(name):
        if name == "links":
            got = ctx.phase_links_lists(recs, words, *sites)
            assert got[0].dtype == np.uint32 and np.array_equal(got[0], links) and np.array_equal(got[1], site_reads), order
        elif name == "tags":
            same(ctx.phase_tags_lists(recs, words, *sites, ps, flip), tags, (order, name))
        else:
            same(seam(ctx, h), rows, (order, name))
        assert launches(ctx).get("k_ph_obs") == 3, (order, name, launches(ctx))

    for order in (("links", "tags", "counts"), ("counts", "links", "tags"), ("tags", "counts", "links")):
        for name in order:
            run(name)


def raw_lists(c, case, cap, rows, n_rows, recs=None, words=None, null=(), n_bases=None):
    """vga_haplotype_counts_lists itself: the return code; rows and n_rows are the caller's"""
    b = pkg().binding
    if recs is None:
        recs, words = P.pack(case.reads)
    rc = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 3)
    wd = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    arrays = {"pos": u32(case.pos), "x": u8(case.x), "y": u8(case.y), "ref": u8(case.ref), "ps": u32(case.ps), "flip": u8(case.flip), "cpos": u32(case.cpos),
              "cref": u8(case.cref)}
    ptr = lambda k: None if k in null else arrays[k].ctypes.data_as(C.POINTER(C.c_uint32 if arrays[k].dtype == np.uint32 else C.c_uint8))
    pad = lambda a: a if a.size else np.zeros(3, dtype=np.uint32)
    return c.L.vga_haplotype_counts_lists(c.h, case.n_bases if n_bases is None else n_bases, len(rc), b._u32p(pad(rc)), len(wd), b._u32p(pad(wd)), len(case.cpos),
                                          ptr("cpos"), ptr("cref"), len(case.pos), ptr("pos"), ptr("x"), ptr("y"), ptr("ref"), ptr("ps"), ptr("flip"), cap,
                                          None if rows is None else b._u32p(rows), None if n_rows is None else C.byref(n_rows))


def test_seam_cap_below_the_jobs_counts_nothing(ctx):
    h = H.HAND
    for cap in (0, 1, 9):
        rows, n_rows = np.full((16, 16), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        assert raw_lists(ctx, h, cap, rows, n_rows) == 0
        assert n_rows.value == 10 and (rows == 0xDEADBEEF).all(), cap
        assert not any(k.startswith("k_") for k in launches(ctx)), (cap, launches(ctx))
    n_rows = C.c_uint64(77)
    assert raw_lists(ctx, h, 0, None, n_rows) == 0 and n_rows.value == 10     # cap 0 needs no rows array
    for cap in (10, 12):
        rows, n_rows = np.full((16, 16), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        assert raw_lists(ctx, h, cap, rows, n_rows) == 0 and n_rows.value == 10
        assert rows[:10].tolist() == H.HAND_ROWS and (rows[10:] == 0xDEADBEEF).all(), cap
    for cap in (0, 9, 10):
        assert seam(ctx, h, cap=cap).tolist() == H.HAND_ROWS, cap


def test_seam_nothing_to_count(ctx):
    h = H.HAND
    recs, words = P.pack(h.reads)
    none = ctx.haplotype_counts_lists(np.zeros((0, 3), dtype=np.uint32), [], h.n_bases, h.cpos, h.cref, h.pos, h.x, h.y, h.ref, h.ps, h.flip)
    assert none.shape == (0, 16) and none.dtype == np.uint32
    assert ctx.haplotype_counts_lists(recs, words, h.n_bases, [], [], h.pos, h.x, h.y, h.ref, h.ps, h.flip).shape == (0, 16)
    assert ctx.haplotype_counts_lists(recs, words, h.n_bases, h.cpos, h.cref, [], [], [], [], [], []).shape == (0, 16)
    assert seam(ctx, h._replace(cpos=[2, 35], cref=[0, 1])).shape == (0, 16)             # calls outside every set: no job
    got = seam(ctx, h._replace(reads=[([(6, 9)], [(7, H.T)])] * 3))                        # reads that consume no site: jobs, and nothing counted
    assert got[:, :2].tolist() == [list(j) for j in H.HAND_JOBS] and not got[:, 2:].any()


def test_seam_refusals_leave_the_outputs_alone(ctx):
    """everything vga_phase_tags_lists refuses and what the calls add: VGA_ERR_ARG, nothing launched, rows and n_rows untouched, the
    context usable afterwards"""
    t = H.HAND
    recs, words = P.pack(t.reads)

    def refused(null=(), no_rows=False, no_count=False, code=-1, **changes):
        case = t._replace(**{k: v for k, v in changes.items() if k in t._fields})
        rows, n_rows = np.full((16, 16), 0xDEADBEEF, dtype=np.uint32), C.c_uint64(77)
        rc = raw_lists(ctx, case, 16, None if no_rows else rows, None if no_count else n_rows, recs=changes.get("recs", recs), words=changes.get("words", words),
                       null=null)
        assert rc == code, (rc, changes, null)
        assert (rows == 0xDEADBEEF).all() and n_rows.value == 77
        assert seam(ctx, t).tolist() == H.HAND_ROWS

    one = lambda ws, n_runs, n_sparse: dict(recs=[[0, n_runs, n_sparse]], words=ws)
    refused(**one([3 << 1], 1, 0))                         # a run word without its partner
    refused(**one([5 << 1, (3 << 1) | 1], 2, 0))           # end below start
    refused(**one([5 << 1, (41 << 1) | 1], 2, 0))          # end behind the graph
    refused(**one([(40 << 3) | 1], 0, 1))                  # sparse position behind the graph
    refused(**one([(3 << 3) | 7], 0, 1))                   # column 7
    refused(recs=[[2, 0, 1]], words=[0, 0])                # the record starts behind the words
    refused(pos=[5, 10, 30, 20])                           # sites descend
    refused(pos=[5, 10, 20, 40])                           # a site behind the graph
    refused(x=[0, 0, 1, 0])                                # x = y
    refused(y=[1, 1, 1, 5])                                # y above D
    refused(ref=[0, 0, 0, 5])                              # own letter above "other"
    refused(ps=[0, 2, 1, 2])                               # no set 0
    refused(ps=[1, 3, 3, 2])                               # a set named by a later site
    refused(ps=[1, 2, 1, 5])                               # a set named by a site that does not exist
    refused(ps=[1, 1, 2, 2])                               # site 1 does not open a set
    refused(flip=[0, 0, 2, 0])                             # flip above 1
    refused(cpos=[2, 5, 7, 10, 10, 20, 25, 30, 35])        # calls do not ascend strictly
    refused(cpos=[2, 5, 7, 10, 15, 20, 25, 35, 30])        # calls descend
    refused(cpos=[2, 5, 7, 10, 15, 20, 25, 30, 40])        # a call behind the graph
    refused(cref=[0, 0, 2, 0, 5, 0, 3, 0, 1])              # own letter of a call above "other"
    for k in ("pos", "x", "y", "ref", "ps", "flip", "cpos", "cref"):
        refused(null=(k,))                                 # a NULL array with a non-zero count
    refused(no_rows=True)                                  # room for rows and no array
    refused(no_count=True)


# ---- 2. through a context, and 3. the executable, on one sample
@pytest.fixture(scope="module")
def sample(oracle, drb1):
    """300 reads of 400 bases from the paths of DRB1, the oracle's alignments GAF of them and everything the reference makes of it"""
    reads = pkg().readsim.simulate_reads(DRB1, 300, 400, 0.02, 0.01, 0.01, seed=61)
    a = oracle_index_arrays(drb1)
    _, gaf, _ = oracle.map_reads(drb1, [r.name for r in reads], [r.seq for r in reads])
    g = ref.gaf(gaf, a["node_seq_idx"], a["seq_fwd"])
    rows = np.array(g["rows"], dtype=np.uint32).reshape(-1, 16)
    assert len(g["shows"]) == len(reads) and len(rows) > 100 and rows[:, 2:9].sum() > 0 and rows[:, 9:].sum() > 0
    assert len(g["cpos"]) > len(g["pos"]) > 10, "calls that are no sites"
    return dict(g, reads=reads, arrays=a, gaf=gaf, table=rows)


def test_context_equals_the_reference(ctx, drb1, sample, monkeypatch):
    p = pkg()
    a = sample["arrays"]
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
    assert v["pos"].tolist() == sample["cpos"] and pos.tolist() == sample["pos"]
    links, _, n_reads = ctx.phase_links(pos, x, y)
    ps, flip, _ = p.binding.phase_chain(links)
    assert ps.tolist() == sample["ps"] and flip.tolist() == sample["flip"]
    rows, n = ctx.haplotype_counts(v["pos"], pos, x, y, ps, flip)
    assert n == len(seqs)
    n_k = launches(ctx)
    assert n_k.get("k_ph_obs") == n_k.get("k_hc_tags") == n_k.get("k_hc_cols") == n_k.get("k_hc_count") == 1, n_k
    same(rows, sample["table"], "the context's store")
    assert p.binding.haplotype_jobs(v["pos"], pos, ps).tolist() == rows[:, :2].tolist()
    same(ctx.haplotype_counts(v["pos"], pos, x, y, ps, flip, cap=1)[0], sample["table"], "asked again")
    recs, words = ctx.phase_reads()
    lists = ctx.haplotype_counts_lists(recs, words, len(a["seq_fwd"]), v["pos"], ref.cref_of(a["seq_fwd"], v["pos"]), pos, x, y,
                                       ref.cref_of(a["seq_fwd"], pos), ps, flip)
    assert np.array_equal(lists, rows)
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    assert np.array_equal(ctx.haplotype_counts(v["pos"], pos, x, y, ps, flip)[0], rows)
    assert launches(ctx).get("k_hc_count") == 5
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    # the tags are those of vga_phase_tags: the store is not reset by either call
    assert len(ctx.phase_tags(pos, x, y, ps, flip)[0]) > 0
    for bad in (dict(ps=np.zeros_like(ps)), dict(cpos=v["pos"][::-1].copy())):
        with pytest.raises(p.VgaError) as e:
            ctx.haplotype_counts(bad.get("cpos", v["pos"]), pos, x, y, bad.get("ps", ps), flip)
        assert e.value.code == -1
    ctx.phase_reset()
    assert ctx.haplotype_counts(v["pos"], pos, x, y, ps, flip)[0].shape == (0, 16)
    ctx.phase_end()
    with pytest.raises(p.VgaError) as e:
        ctx.haplotype_counts(v["pos"], pos, x, y, ps, flip)
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
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1, "--call-variants", "--phase", "--haplotag"]
    pr = run(common + ["-o", os.path.join(d, "plain")])
    assert not os.path.exists(os.path.join(d, "plain-haplotype-calls.tsv")) and "haplotype-calls" not in pr.stderr
    read = lambda name: open(os.path.join(d, name)).read()
    assert read("plain-alignments.gaf") == sample["gaf"]
    want, n_jobs, n_lines, differ = ref.tsv(sample["rows"], sample["cpos"], a["node_seq_idx"], a["seq_fwd"])
    assert n_jobs == len(sample["rows"]) and 0 < n_lines <= n_jobs and differ > 0
    for out, extra in (("one", []), ("chunks", ["--chunk-reads", "10"]), ("two", ["--devices", "0,0", "--chunk-reads", "10"])):
        pr = run(common + ["-o", os.path.join(d, out), "--haplotype-calls"] + extra)
        assert read(out + "-haplotype-calls.tsv") == want, out
        assert "haplotype-calls: %d jobs, %d rows, %d differ" % (n_jobs, n_lines, differ) in pr.stderr, pr.stderr
        # every other file is byte for byte what it is without the switch
        files = {f[len(out):] for f in os.listdir(d) if f.startswith(out + "-")}
        assert files == {f[len("plain"):] for f in os.listdir(d) if f.startswith("plain-")} | {"-haplotype-calls.tsv"}
        for suffix in files - {"-haplotype-calls.tsv"}:
            assert read(out + suffix) == read("plain" + suffix), (out, suffix)
    # no heterozygous site: the header only
    pr = run(common + ["-o", os.path.join(d, "none"), "--haplotype-calls", "--call-min-depth", "1000"])
    assert read("none-haplotype-calls.tsv") == ref.HEADER + "\n" and "haplotype-calls: 0 jobs, 0 rows, 0 differ" in pr.stderr
    pr = subprocess.run([EXE] + common[:-1] + ["--haplotype-calls", "-o", os.path.join(d, "bad")], cwd=d, capture_output=True, text=True, timeout=300)
    assert pr.returncode != 0 and "--haplotag" in pr.stderr and not [f for f in os.listdir(d) if f.startswith("bad")]
