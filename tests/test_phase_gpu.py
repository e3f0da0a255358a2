"""The phase store and the phase links on the GPU (vga_phase_begin / _read / _reset / _end / _links / _links_lists, k_ph_keep +
k_ph_obs + k_ph_link, `vgaligner map --call-variants --phase`).  Every comparison is exact equality of the uint32 tables with the
reference (tests/phase_ref.py): through the kernel seam on synthetic lists (tests/phase_cases.py) at the smallest shapes where the
kernels can go wrong, through a context against the reference run over that build's own alignments GAF, and through the
executable.  Without the feature every test here stops at Context.phase_begin / phase_links_lists (no such call) or at the unknown
--phase flag."""
import os
import subprocess

import numpy as np
import pytest

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


def same(got, want, what=""):
    (gl, gs), (wl, ws) = got, want
    assert gl.dtype == np.uint32 and gs.dtype == np.uint32 and gl.shape == wl.shape and gs.shape == ws.shape, (what, gl.shape, wl.shape, gs.shape, ws.shape)
    bad = np.argwhere(gl != wl)
    assert len(bad) == 0, (what, "links", len(bad), bad[:8].tolist(), [int(gl[tuple(i)]) for i in bad[:8]], [int(wl[tuple(i)]) for i in bad[:8]])
    bad = np.argwhere(gs != ws)
    assert len(bad) == 0, (what, "site_reads", len(bad), bad[:8].tolist(), [int(gs[tuple(i)]) for i in bad[:8]], [int(ws[tuple(i)]) for i in bad[:8]])


def seam(c, case):
    recs, words = P.pack(case.reads)
    return c.phase_links_lists(recs, words, case.n_bases, case.pos, case.x, case.y, case.ref)


def reference(case):
    recs, words = P.pack(case.reads)
    return phase_ref.tables(phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref), len(case.pos))


# ---- 1. the seam
def test_seam_cases_written_out_by_hand(ctx):
    """runs that start at a site, end at it and end one behind it, a run over several sites, sites at base 0 and at the last base,
    a deletion allele, an N read letter, an insertion word at a site, a site whose own letter is neither allele or no letter,
    bases consumed twice, a read with no word"""
    same(seam(ctx, P.TINY), (P.TINY_LINKS, P.TINY_SITE_READS), "tiny")
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_ph_obs" in names and "k_ph_link" in names, names
    same(seam(ctx, P.EDGE), phase_ref.tables(P.EDGE_OBS, 5), "edge")
    same(seam(ctx, P.EDGE), reference(P.EDGE), "edge, from the lists")


def test_seam_links_eight_apart_and_not_nine(ctx):
    far = P.far_case()
    links, sr = seam(ctx, far)
    same((links, sr), reference(far), "far")
    assert links[0, 7].tolist() == [3, 0, 2, 0] and int(links.sum()) == 5 and sr[9].tolist() == [0, 4, 0]


@pytest.mark.parametrize("n_reads", [1, 63, 64, 65, 129])
def test_seam_read_counts(ctx, n_reads):
    """the ballot's tail and a second wave of k_ph_link"""
    case = P.random_case("reads", n_reads, 10, seed=200 + n_reads)
    want = reference(case)
    assert n_reads == 1 or int(want[0].sum()) > 0
    same(seam(ctx, case), want, "%d reads" % n_reads)


def test_seam_three_tiles_the_last_partial(ctx, monkeypatch):
    case = P.random_case("tiles", 130, 12, seed=7)
    want = reference(case)
    assert int(want[0].sum()) > 100 and all(phase_ref.tables(phase_ref.obs_lists(*P.pack(case.reads[k:k + 64]), case.pos, case.x, case.y, case.ref), 12)[0].any() for k in (0, 64, 128))
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    same(seam(ctx, case), want, "tile of 64")
    launches = {t["name"]: t["launches"] for t in ctx.kernel_times()}
    assert launches.get("k_ph_obs") == 3 and launches.get("k_ph_link") == 3, launches
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    same(seam(ctx, case), want, "one tile")
    launches = {t["name"]: t["launches"] for t in ctx.kernel_times()}
    assert launches.get("k_ph_obs") == 1, launches


@pytest.mark.parametrize("n_sites", [1, 2, 8, 9, 10])
def test_seam_site_counts(ctx, n_sites):
    """h + d < H is cut at every d"""
    case = P.random_case("sites", 70, n_sites, seed=300 + n_sites, n_bases=40)
    want = reference(case)
    assert int(want[1].sum()) > 0 and (n_sites == 1 or int(want[0].sum()) > 0)
    got = seam(ctx, case)
    same(got, want, "%d sites" % n_sites)
    for h in range(n_sites):
        assert not got[0][h, max(0, n_sites - 1 - h):].any(), h


def test_seam_nothing_to_link(ctx):
    links, sr = ctx.phase_links_lists(np.zeros((0, 3), dtype=np.uint32), [], 20, [3, 7], [0, 1], [2, 3], [0, 3])
    assert links.shape == (2, 8, 4) and not links.any() and not sr.any()
    recs, words = P.pack(P.TINY.reads)
    links, sr = ctx.phase_links_lists(recs, words, 20, [], [], [], [])
    assert links.shape == (0, 8, 4) and sr.shape == (0, 3)


def test_seam_refusals(ctx):
    """every index a kernel follows is checked on the host: VGA_ERR_ARG, nothing launched, the context usable afterwards"""
    p = pkg()
    t = P.TINY
    recs, words = P.pack(t.reads)

    def refused(recs=recs, words=words, n_bases=t.n_bases, pos=t.pos, x=t.x, y=t.y, ref=t.ref):
        with pytest.raises(p.VgaError) as e:
            ctx.phase_links_lists(recs, words, n_bases, pos, x, y, ref)
        assert e.value.code == -1, str(e.value)
        same(seam(ctx, t), (P.TINY_LINKS, P.TINY_SITE_READS), "after a refusal")

    one = lambda ws, n_runs, n_sparse: dict(recs=[[0, n_runs, n_sparse]], words=ws)
    refused(**one([3 << 1], 1, 0))                         # a run word without its partner
    refused(**one([(3 << 1) | 1, (5 << 1) | 1], 2, 0))     # two end words
    refused(**one([3 << 1, 5 << 1], 2, 0))                 # two start words
    refused(**one([5 << 1, (5 << 1) | 1], 2, 0))           # end at start
    refused(**one([5 << 1, (3 << 1) | 1], 2, 0))           # end below start
    refused(**one([5 << 1, (21 << 1) | 1], 2, 0))          # end behind the graph
    refused(**one([(20 << 3) | 1], 0, 1))                  # sparse position behind the graph
    refused(**one([(3 << 3) | 7], 0, 1))                   # column 7
    refused(**one([3 << 1, (5 << 1) | 1], 2, 1))           # the record runs past the words
    refused(recs=[[2, 0, 1]], words=[0, 0])                # the record starts behind the words
    refused(pos=[7, 3])                                    # sites descend
    refused(pos=[3, 3])                                    # a site twice
    refused(pos=[3, 20])                                   # a site behind the graph
    refused(x=[2, 1])                                      # x = y
    refused(x=[3, 1])                                      # x above y
    refused(y=[2, 5])                                      # y above D
    refused(ref=[0, 5])                                    # own letter above "other"
    ok = ctx.phase_links_lists([[0, 2, 0]], [19 << 1, (20 << 1) | 1], 20, [19], [0], [4], [0])   # the last base, end = n_bases
    assert ok[1].tolist() == [[1, 0, 0]]


# ---- 2. through a context
def own_gaf(al, seqs):
    """the alignments GAF of an align result, as far as the reference reads it: path, start, end and the cs string"""
    lines = []
    for r, s in enumerate(seqs):
        if not al.aligned[r]:
            lines.append("\t".join(["r%d" % r, str(len(s)), "0", "0", "+", "*", "0", "0", "0", "0", "0", "255", "as:i:0"]))
            continue
        path = "".join(">%d" % (h >> 1) for h in al.path_handles[int(al.path_off[r]):int(al.path_off[r + 1])].tolist())
        lines.append("\t".join(["r%d" % r, str(len(s)), "0", str(len(s)), "+", path, str(int(al.path_length[r])), str(int(al.path_start[r])),
                                str(int(al.path_end[r])), "0", str(int(al.block_length[r])), "60", "as:i:-30 " + al.cs[r] + ",cg:Z:" + al.cigar[r]]))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def two_paths():
    """the reads of paths 2 and 5 among test_genotype_cpu.py's 120 reads of 3 kbp"""
    rs = pkg().readsim
    names = [n for n, _ in rs.parse_gfa_paths(DRB1)[1]]
    seqs = [r.seq for r in rs.simulate_reads(DRB1, 120, 3000, 0.03, 0.03, 0.04, seed=7) if names.index(r.path) in (2, 5)]
    assert len(seqs) == 26
    return seqs


def sites_of(c):
    v = c.variant_call()
    het = np.flatnonzero(v["x"] < v["y"])
    return v["pos"][het], v["x"][het], v["y"][het]


def check_context(c, arrays, gaf, what, n_reads):
    """phase_links at the sites of variant_call against the reference on the GAF; x_reads and y_reads against the pileup (DRB1
    is acyclic: a read consumes a base once); the store fed back through the seam"""
    pos, x, y = sites_of(c)
    assert len(pos) >= 10, len(pos)
    got = c.phase_links(pos, x, y)
    assert got[2] == n_reads
    names = [t["name"] for t in c.kernel_times()]
    assert "k_ph_obs" in names and "k_ph_link" in names, names
    want = phase_ref.links_gaf(gaf, arrays["node_seq_idx"], arrays["seq_fwd"], pos.tolist(), x.tolist(), y.tolist())
    assert int(want[0].sum()) > 0
    same(got[:2], want, what)
    pu = c.pileup()[0]
    col = lambda a: np.where(a == 4, 5, a)   # allele D is the pileup's del column
    assert np.array_equal(got[1][:, 0], pu[pos, col(x)]) and np.array_equal(got[1][:, 1], pu[pos, col(y)]), what
    recs, words = c.phase_reads()
    assert len(recs) == n_reads and int(recs[:, 1].sum() + recs[:, 2].sum()) == len(words)
    ref = [phase_ref.allele(chr(arrays["seq_fwd"][int(p)])) for p in pos]
    ref = [r if r < 4 else 4 for r in ref]
    same(c.phase_links_lists(recs, words, len(arrays["seq_fwd"]), pos, x, y, ref), want, what + ", through the seam")
    return got


ROUTES = [{}, {"VGA_PILEUP_LIST_WORDS": "0"}, {"VGA_PHASE_STORE_WORDS": "64", "calls": 3}, {"calls": 3}, {"both_strands": True}, {"best_n": 2}]


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: ",".join("%s=%s" % kv for kv in r.items()) or "defaults")
def test_context_equals_the_reference(ctx, drb1, two_paths, monkeypatch, capfd, route):
    """the lists of the device and those the host builds (VGA_PILEUP_LIST_WORDS=0), a store that has to grow in every batch, three
    align calls, reads given as reverse complements, two candidates per read: the library's trace says which route was taken"""
    p = pkg()
    monkeypatch.setenv("VGA_TRACE", "1")
    rs = p.readsim
    route = dict(route)
    calls, both, best_n = route.pop("calls", 1), route.pop("both_strands", False), route.pop("best_n", 1)
    for k, v in route.items():
        monkeypatch.setenv(k, v)
    seqs = [rs.reverse_complement(s) if both and i % 2 == 0 else s for i, s in enumerate(two_paths)]
    mp = p.default_map_params()
    if both:
        mp.strands = p.binding.VGA_STRANDS_BOTH
    arrays = oracle_index_arrays(drb1)
    upload_oracle_index(ctx, drb1)
    ctx.pileup_begin()
    ctx.phase_begin()
    capfd.readouterr()
    gaf, n_aligned, kept = "", 0, False
    for k in range(calls):
        part = seqs[k * len(seqs) // calls:(k + 1) * len(seqs) // calls]
        b = ctx.batch(part)
        al = b.align(b.map(mp), best_n=best_n)
        b.close()
        kept = kept or "k_ph_keep" in [t["name"] for t in ctx.kernel_times()]
        gaf += own_gaf(al, part)
        n_aligned += int(al.aligned.sum())
    assert kept and n_aligned == len(seqs)
    trace = capfd.readouterr().err
    by_host, grown = trace.count("no room for its pileup list"), trace.count("phase: the store grows")
    print("lists built by the host", by_host, "growths", grown)
    assert by_host == (len(seqs) if "VGA_PILEUP_LIST_WORDS" in route else 0)
    # from 64 words the store doubles past the first batch's words, so a later batch of as many words moves what is stored; from
    # 2^20 words it is allocated once
    assert grown >= 2 if "VGA_PHASE_STORE_WORDS" in route else grown == 1
    check_context(ctx, arrays, gaf, str(route) + str((calls, both, best_n)), n_aligned)
    ctx.phase_end()
    ctx.pileup_end()


def test_life_cycle(drb1, two_paths, oracle):
    p = pkg()
    arrays = oracle_index_arrays(drb1)
    seqs = two_paths[:8]

    def align(c):
        b = c.batch(seqs)
        al = b.align(b.map())
        b.close()
        return al

    c = p.Context(0)
    try:
        with pytest.raises(p.VgaError) as e:
            c.phase_begin()
        assert e.value.code == -5  # VGA_ERR_NO_INDEX
        upload_oracle_index(c, drb1)
        with pytest.raises(p.VgaError) as e:
            c.phase_begin()
        assert e.value.code == -1 and "pileup" in str(e.value)  # begin without the pileup
        for call in (c.phase_reads, c.phase_reset, lambda: c.phase_links([0], [0], [1])):
            with pytest.raises(p.VgaError) as e:
                call()
            assert e.value.code == -1
        c.pileup_begin()
        align(c)
        assert not any(t["name"].startswith("k_ph") for t in c.kernel_times()), "store off: no phase kernel"
        c.phase_begin()
        assert len(c.phase_reads()[0]) == 0
        al = align(c)
        first = c.phase_reads()
        assert len(first[0]) == int(al.aligned.sum()) == len(seqs) and len(first[1]) > 0
        align(c)
        twice = c.phase_reads()
        assert len(twice[0]) == 2 * len(seqs) and len(twice[1]) == 2 * len(first[1])
        assert np.array_equal(twice[1][:len(first[1])], first[1]) and np.array_equal(twice[1][len(first[1]):], first[1])
        assert np.array_equal(twice[0][len(seqs):, 0], first[0][:, 0] + len(first[1])) and np.array_equal(twice[0][len(seqs):, 1:], first[0][:, 1:])
        c.phase_reset()
        assert len(c.phase_reads()[0]) == 0 and len(c.phase_reads()[1]) == 0
        links, sr, n = c.phase_links([100, 200], [0, 1], [1, 2])
        assert n == 0 and not links.any() and not sr.any()
        align(c)
        again = c.phase_reads()
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1])
        c.phase_end()
        with pytest.raises(p.VgaError) as e:
            c.phase_reads()
        assert e.value.code == -1
        align(c)
        assert not any(t["name"].startswith("k_ph") for t in c.kernel_times())
        c.phase_begin()  # end, then begin: an empty store
        assert len(c.phase_reads()[0]) == 0
        align(c)
        assert np.array_equal(c.phase_reads()[1], first[1])
        for bad in (dict(pos=[5, 5]), dict(pos=[len(arrays["seq_fwd"])]), dict(x=[1], y=[1]), dict(y=[5])):
            args = dict(pos=[5], x=[0], y=[1])
            args.update(bad)
            args = {k: v * len(args["pos"]) if len(v) != len(args["pos"]) else v for k, v in args.items()}
            with pytest.raises(p.VgaError) as e:
                c.phase_links(args["pos"], args["x"], args["y"])
            assert e.value.code == -1, bad
        # a new index releases the store
        upload_oracle_index(c, oracle.Index(oracle.Graph.from_gfa(DRB1), 19))
        with pytest.raises(p.VgaError) as e:
            c.phase_reads()
        assert e.value.code == -1
        c.phase_end()
        c.phase_end()  # (ending twice is harmless)
    finally:
        c.close()


# ---- 3. the executable
def test_cli(oracle, drb1, tmp_path):
    p = pkg()
    d = str(tmp_path)
    a = oracle_index_arrays(drb1)
    reads, at, new, old = P.planted_sample(p.readsim, DRB1, a["node_seq_idx"])
    fa = os.path.join(d, "r.fa")
    with open(fa, "w") as f:
        for name, seq in reads:
            f.write(">%s\n%s\n" % (name, seq))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain"), "--call-variants", "--call-insertions"])
    assert not os.path.exists(os.path.join(d, "plain-phase.tsv"))
    read = lambda name: open(os.path.join(d, name)).read()
    gaf = read("plain-alignments.gaf")
    want, sites, sets, n_records = phase_ref.tsv_gaf(gaf, a["node_seq_idx"], a["seq_fwd"])
    assert sites >= 3 and n_records == len(reads)
    # the planted phase, in the file: the three sites in one set, s1 and s3 against s2
    idx = [int(v) for v in a["node_seq_idx"]]
    rows = {}
    for line in want.splitlines()[1:]:
        f = line.split("\t")
        rows[idx[int(f[0]) - 1] + int(f[1])] = f
    assert all(g in rows for g in at) and len({rows[g][3] for g in at}) == 1
    hap_a = [rows[g][2][0] for g in at]
    assert hap_a in ([new[0], old[1], new[2]], [old[0], new[1], old[2]])
    for out, extra in (("one", []), ("chunks", ["--chunk-reads", "8"]), ("two", ["--devices", "0,0", "--chunk-reads", "8"])):
        pr = run(common + ["-o", os.path.join(d, out), "--call-variants", "--call-insertions", "--phase"] + extra)
        assert read(out + "-phase.tsv") == want, out
        assert "phase: %d heterozygous sites, %d phase sets, %d reads kept" % (sites, sets, n_records) in pr.stderr, pr.stderr
        # every other file is byte for byte what it is without the switch
        files = {f[len(out):] for f in os.listdir(d) if f.startswith(out + "-")}
        assert files == {f[len("plain"):] for f in os.listdir(d) if f.startswith("plain-")} | {"-phase.tsv"}
        for suffix in files - {"-phase.tsv"}:
            assert read(out + suffix) == read("plain" + suffix), (out, suffix)
    # no heterozygous site: the header only
    pr = run(common + ["-o", os.path.join(d, "none"), "--call-variants", "--phase", "--call-min-depth", "1000"])
    assert read("none-phase.tsv") == phase_ref.HEADER + "\n" and "phase: 0 heterozygous sites, 0 phase sets, %d reads kept" % n_records in pr.stderr
    pr = subprocess.run([EXE] + common + ["-o", os.path.join(d, "bad"), "--phase"], cwd=d, capture_output=True, text=True, timeout=300)
    assert pr.returncode != 0 and "--call-variants" in pr.stderr and not [f for f in os.listdir(d) if f.startswith("bad")]
