"""The haplotype paths on the GPU (vga_haplotype_paths / vga_haplotype_paths_lists: k_ph_obs + k_hc_tags + k_hp_sums; the deficit store
of k_hp_keep; `vgaligner map --call-variants --phase --haplotype-paths`).  Every comparison is exact equality of the uint64 reads and
table with the reference (tests/haplotype_paths_ref.py): through the kernel seam on synthetic lists (tests/haplotype_paths_cases.py)
at the smallest shapes where the kernels can go wrong, through a context against the reference run over the oracle's alignments GAF,
and through the executable.  Without the feature every test here stops at Context.haplotype_paths_lists / haplotype_paths_begin (no
such call) or at the unknown --haplotype-paths flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import haplotype_calls_ref as hc_ref
import haplotype_paths_cases as K
import haplotype_paths_ref as ref
import path_support_ref
import phase_cases as P
import phase_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
KERNELS = ("k_ph_obs", "k_hc_tags", "k_hp_sums")


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


def seam(c, k, ps=None, flip=None):
    t = k.case
    recs, words = P.pack(t.reads)
    return c.haplotype_paths_lists(recs, words, t.n_bases, k.deficits, k.scored, t.pos, t.x, t.y, t.ref, k.ps if ps is None else ps, k.flip if flip is None else flip)


def launches(c):
    return {t["name"]: t["launches"] for t in c.kernel_times()}


def check(c, k, what=None):
    want_reads, want_table = ref.sums(obs_of(k.case), k.ps, k.flip, k.deficits, k.scored)
    reads, table, n_sets = seam(c, k)
    assert n_sets == len(set(k.ps)), what or k.name
    ref.same(reads, table, want_reads, want_table, what or k.name)
    return want_reads, want_table


# ---- 1. the seam
def test_seam_cases_written_out_by_hand(ctx):
    reads, table, n_sets = seam(ctx, K.TINY)
    assert n_sets == 2 and reads.tolist() == K.TINY_READS and table[:, :, 0].tolist() == K.TINY_COST and table[:, :, 1].tolist() == K.TINY_BEST
    n = launches(ctx)
    assert all(n.get(k) == 1 for k in KERNELS), n
    assert not any(k in n for k in ("k_ph_link", "k_ph_tag", "k_hc_cols", "k_hc_count", "k_sj_bits", "k_sj_pairs", "k_hp_keep")), n
    reads, table, n_sets = seam(ctx, K.TINY_ONE)
    assert n_sets == 1 and reads.tolist() == K.TINY_ONE_READS and table[:, :, 0].tolist() == K.TINY_ONE_COST and table[:, :, 1].tolist() == K.TINY_ONE_BEST
    # a row of all-equal scores: every path is best
    one = K.HpCase("equal", P.Case("equal", 8, [3], [P.A], [P.C], [P.G], [([], [(3, P.A)])]), [1], [0], np.zeros((1, 4), dtype=np.uint8), [1])
    reads, table, _ = seam(ctx, one)
    assert reads.tolist() == [1, 0] and table[0].tolist() == [[0, 1]] * 4 and not table[1].any()


@pytest.mark.parametrize("n_reads", [11, 70, 127])
def test_seam_tags_of_every_kind_in_every_lane(ctx, n_reads):
    """a read tagged in no set, one tied in a set and tagged in the other, an unscored read that is tagged, in every lane position
    of the last, partial word: six shifts of a pattern of period six"""
    for shift in range(6):
        k, kind = K.kinds_case(n_reads, shift)
        want_reads, want_table = K.kinds_groups(kind)
        reads, table, n_sets = seam(ctx, k)
        assert n_sets == 2
        ref.same(reads, table, want_reads, want_table, (n_reads, shift))
        check(ctx, k, (n_reads, shift))


@pytest.mark.parametrize("n_paths", K.PATH_COUNTS)
def test_seam_path_counts(ctx, n_paths):
    """around the pitch of four bytes, a lane's four paths, a wave's word of 64 and a workgroup's chunk of 256 paths; the unscored
    reads carry rows that are not zero"""
    k = K.paths_case(n_paths)
    want_reads, want_table = check(ctx, k)
    assert want_reads.sum() > 0 and want_table[:, -1, :].sum() > 0 and (np.asarray(k.deficits)[np.asarray(k.scored) == 0] != 0).any()


@pytest.mark.parametrize("n_reads", K.READ_COUNTS)
def test_seam_read_counts_and_tiles(ctx, monkeypatch, n_reads):
    """the edges of the ballot word, under tiles of 64 reads (129 reads: a last tile of one read, shorter than a word) and under the
    default tile: identical tables"""
    k = K.paths_case(65, n_reads=n_reads, n_sites=10, n_sets=4)
    reads = list(k.case.reads)
    for r in {0, n_reads - 1, min(63, n_reads - 1), min(64, n_reads - 1)}:
        reads[r] = ([(0, k.case.n_bases)], [])   # a read over every site at the edges of the words
    k = k._replace(case=k.case._replace(reads=reads))
    want_reads, want_table = check(ctx, k)
    tiles = (n_reads + 63) // 64
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    reads_small, table_small, _ = seam(ctx, k)
    n = launches(ctx)
    assert all(n.get(name) == tiles for name in KERNELS), n
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    ref.same(reads_small, table_small, want_reads, want_table, "tiles of 64")
    assert n_reads < 63 or want_reads.sum() > 0


@pytest.mark.parametrize("n_sets", K.SET_COUNTS)
def test_seam_set_counts(ctx, n_sets):
    k = K.sets_case(n_sets)
    want_reads, _ = check(ctx, k)
    assert len(want_reads) == 2 * n_sets and len(set(k.ps)) == n_sets
    for s in (0, n_sets // 2, n_sets - 1):
        assert want_reads[2 * s] + want_reads[2 * s + 1] >= 1, s


@pytest.mark.parametrize("cap", [1, 64, 255])
def test_seam_rows_at_the_cap_and_of_64_bit_scores(ctx, cap):
    """deficits of exactly cap - 1, cap and above and a row whose bases + edges passes 2^32 (the rule of the store, here from the
    reference, which tests/test_haplotype_paths_cpu.py checks by hand), summed"""
    bases, edges = K.wide_scores()
    d, scored = ref.deficits(bases, edges, cap)
    assert d.tolist() == K.WIDE_DEFICITS[cap]
    case = P.Case("wide", 12, [3, 7], [P.A, P.A], [P.C, P.C], [P.G, P.G], [([], [(3, P.A), (7, P.C)])] * 3 + [([], [(3, P.C)])] * 2)
    k = K.HpCase("wide", case, [1, 2], [0, 0], d, scored)
    want_reads, want_table = check(ctx, k)
    assert want_reads.tolist() == [3, 1, 0, 3] and int(want_table[:, :, 0].max()) <= 3 * cap   # (read 4 is unscored)


def test_seam_nothing_to_sum(ctx):
    t = K.TINY.case
    recs, words = P.pack(t.reads)
    reads, table, n_sets = ctx.haplotype_paths_lists(np.zeros((0, 3), dtype=np.uint32), [], t.n_bases, np.zeros((0, 3), dtype=np.uint8), [], t.pos, t.x, t.y, t.ref,
                                                     [1, 2], [0, 0])
    assert reads.shape == (0,) and table.shape == (0, 3, 2) and n_sets == 0                        # an empty store
    assert not any(k.startswith("k_") for k in launches(ctx))
    reads, table, n_sets = ctx.haplotype_paths_lists(recs, words, t.n_bases, K.TINY_DEFICITS, K.TINY_SCORED, [], [], [], [], [], [])
    assert reads.shape == (0,) and n_sets == 0                                                     # no site
    assert not any(k.startswith("k_") for k in launches(ctx))
    far = K.TINY._replace(case=t._replace(reads=[([(12, 19)], [(15, P.T)])] * 6))                  # reads that consume no site
    reads, table, n_sets = seam(ctx, far)
    assert n_sets == 2 and reads.tolist() == [0, 0, 0, 0] and table.shape == (4, 3, 2) and not table.any()


def raw_lists(c, k, cap_groups, reads, table, n_sets, n_paths=None, null=(), scored=None, ps=None, flip=None, case=None):
    """vga_haplotype_paths_lists itself: the return code; reads, table and n_sets are the caller's"""
    b = pkg().binding
    t = case or k.case
    recs, words = P.pack(t.reads)
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    u8 = lambda a: np.ascontiguousarray(a, dtype=np.uint8)
    arrays = {"pos": u32(t.pos), "x": u8(t.x), "y": u8(t.y), "ref": u8(t.ref), "ps": u32(k.ps if ps is None else ps), "flip": u8(k.flip if flip is None else flip),
              "deficits": u8(k.deficits), "scored": u8(k.scored if scored is None else scored)}
    ptr = lambda name: None if name in null else arrays[name].ctypes.data_as(C.POINTER(C.c_uint32 if arrays[name].dtype == np.uint32 else C.c_uint8))
    pad = lambda a: a if a.size else np.zeros(3, dtype=np.uint32)
    return c.L.vga_haplotype_paths_lists(c.h, t.n_bases, len(recs), b._u32p(pad(recs)), len(words), b._u32p(pad(words)),
                                         arrays["deficits"].shape[1] if n_paths is None else n_paths, ptr("deficits"), ptr("scored"), len(t.pos), ptr("pos"), ptr("x"),
                                         ptr("y"), ptr("ref"), ptr("ps"), ptr("flip"), cap_groups, None if reads is None else b._u64p(reads),
                                         None if table is None else b._u64p(table), None if n_sets is None else C.byref(n_sets))


FILL = 0xDEADBEEFDEADBEEF


def outputs():
    return np.full(8, FILL, dtype=np.uint64), np.full((8, 3, 2), FILL, dtype=np.uint64), C.c_uint64(77)


def quiet(c):
    """a call that launches nothing: from here on the context reports no kernel, until one is launched"""
    n_sets = C.c_uint64(0)
    assert raw_lists(c, K.TINY, 0, None, None, n_sets) == 0 and n_sets.value == 2
    assert not any(k.startswith("k_") for k in launches(c)), launches(c)


def test_seam_cap_below_the_groups_sums_nothing(ctx):
    for cap in (0, 3):
        reads, table, n_sets = outputs()
        assert raw_lists(ctx, K.TINY, cap, reads, table, n_sets) == 0
        assert n_sets.value == 2 and (reads == FILL).all() and (table == FILL).all(), cap
        assert not any(k.startswith("k_") for k in launches(ctx)), (cap, launches(ctx))
    for cap in (4, 8):
        reads, table, n_sets = outputs()
        assert raw_lists(ctx, K.TINY, cap, reads, table, n_sets) == 0 and n_sets.value == 2
        assert reads[:4].tolist() == K.TINY_READS and (reads[4:] == FILL).all(), cap
        assert table[:4, :, 0].tolist() == K.TINY_COST and table[:4, :, 1].tolist() == K.TINY_BEST and (table[4:] == FILL).all()


def test_seam_refusals_leave_the_outputs_alone(ctx):
    """what vga_phase_tags_lists refuses, what this call adds to it, more than 4096 sets and a table above 2^23 entries: nothing
    launched, reads and table untouched, the context usable afterwards"""
    def refused(code=-1, wrote_sets=None, **how):
        reads, table, n_sets = outputs()
        quiet(ctx)
        no = how.pop("no", ())
        rc = raw_lists(ctx, how.pop("k", K.TINY), how.pop("cap", 8), None if "reads" in no else reads, None if "table" in no else table, None if "n_sets" in no else n_sets,
                       **how)
        assert rc == code, (rc, how)
        assert (reads == FILL).all() and (table == FILL).all() and n_sets.value == (77 if wrote_sets is None else wrote_sets)
        assert not any(k.startswith("k_") for k in launches(ctx)), launches(ctx)
        assert seam(ctx, K.TINY)[0].tolist() == K.TINY_READS

    refused(n_paths=0)
    refused(n_paths=4097)
    refused(scored=[1, 1, 2, 0, 1, 0])                     # scored above 1
    refused(ps=[0, 2])                                     # no set 0
    refused(ps=[1, 3])                                     # a set named by a site that does not exist
    refused(flip=[0, 2])                                   # flip above 1
    refused(case=K.TINY.case._replace(pos=[7, 3]))         # sites descend
    refused(case=K.TINY.case._replace(x=[P.G, P.C]))       # x = y
    refused(case=K.TINY.case._replace(ref=[5, 0]))         # own letter above "other"
    for name in ("pos", "x", "y", "ref", "ps", "flip", "deficits", "scored"):
        refused(null=(name,))                              # a NULL array with a non-zero count
    for name in ("reads", "table", "n_sets"):
        refused(no=(name,))                                # room for groups and no array
    # 4097 singleton sets: refused with the count, before anything is launched
    n = 4097
    many = P.Case("many", 2 * n + 2, [2 * h for h in range(n)], [P.A] * n, [P.C] * n, [P.G] * n, [([(0, 9)], [])])
    k = K.HpCase("many", many, [h + 1 for h in range(n)], [0] * n, np.zeros((1, 3), dtype=np.uint8), [1])
    refused(code=-4, wrote_sets=n, k=k, cap=0)
    with pytest.raises(pkg().VgaError) as e:
        seam(ctx, k)
    assert e.value.code == -4 and "4097" in str(e.value), str(e.value)
    # 1025 sets of 4096 paths: 2 S n_paths = 2^23 + 8192 entries; 1024 sets are 2^23 exactly and would be served (not asked for here)
    n = 1025
    wide = P.Case("wide", 2 * n + 2, [2 * h for h in range(n)], [P.A] * n, [P.C] * n, [P.G] * n, [([(0, 9)], [])])
    k = K.HpCase("wide", wide, [h + 1 for h in range(n)], [0] * n, np.zeros((1, 4096), dtype=np.uint8), [1])
    refused(code=-4, wrote_sets=n, k=k, cap=0)
    with pytest.raises(pkg().VgaError) as e:
        seam(ctx, k)
    assert e.value.code == -4 and "1025" in str(e.value) and "4096" in str(e.value), str(e.value)
    n_sets = C.c_uint64(77)
    k = k._replace(case=wide._replace(pos=wide.pos[:-1], x=wide.x[:-1], y=wide.y[:-1], ref=wide.ref[:-1]), ps=k.ps[:-1], flip=k.flip[:-1])
    assert raw_lists(ctx, k, 0, None, None, n_sets) == 0 and n_sets.value == 1024 and not any(name.startswith("k_") for name in launches(ctx))


# ---- 2. through a context, and 3. the executable, on one sample
@pytest.fixture(scope="module")
def sample(oracle, drb1):
    """300 reads of 400 bases from the paths of DRB1, the oracle's alignments GAF of them and everything the reference makes of it"""
    reads = pkg().readsim.simulate_reads(DRB1, 300, 400, 0.02, 0.01, 0.01, seed=61)
    a = oracle_index_arrays(drb1)
    _, gaf, _ = oracle.map_reads(drb1, [r.name for r in reads], [r.seq for r in reads])
    g = ref.gaf(gaf, DRB1, a["node_seq_idx"], a["seq_fwd"])
    assert len(g["obs"]) == len(reads) and g["n_sets"] > 3 and len(g["ranked"]) > 3 and g["scored"].sum() > 200
    return dict(g, sim=reads, arrays=a, gaf=gaf)


def begin(c, drb1, edit=False):
    p = pkg()
    upload_oracle_index(c, drb1)
    _, paths = path_support_ref.parse_gfa(DRB1)
    c.path_support_begin(*path_support_ref.packed_steps(paths))
    if edit:
        c.path_edit_begin()
    c.pileup_begin()
    c.phase_begin()
    return p


def align(c, seqs):
    b = c.batch(seqs)
    al = b.align(b.map())
    b.close()
    assert int(al.aligned.sum()) == len(seqs)


def test_context_equals_the_reference(ctx, drb1, sample, monkeypatch):
    p = begin(ctx, drb1)
    seqs = [r.seq for r in sample["sim"]]
    # the switch off: no k_hp_* launch
    align(ctx, seqs[:40])
    assert not any(k.startswith("k_hp") for k in launches(ctx)), launches(ctx)
    with pytest.raises(p.VgaError) as e:
        ctx.haplotype_paths_store()
    assert e.value.code == -1
    # a store that is turned on behind kept reads never lines up with them: every reader refuses
    ctx.haplotype_paths_begin()
    align(ctx, seqs[40:60])
    assert launches(ctx).get("k_hp_keep") == 1
    v = ctx.variant_call()
    het = np.flatnonzero(v["x"] < v["y"])
    for read in (ctx.haplotype_paths_store, lambda: ctx.haplotype_paths(v["pos"][het], v["x"][het], v["y"][het], np.arange(1, len(het) + 1), np.zeros(len(het)))):
        with pytest.raises(p.VgaError) as e:
            read()
        assert e.value.code == -1 and "20 rows" in str(e.value) and "60 reads" in str(e.value), str(e.value)
    # phase_reset empties both stores; the store grows from one row across three calls
    ctx.pileup_reset()
    ctx.phase_reset()
    d, sc = ctx.haplotype_paths_store()
    assert d.shape[0] == 0 and sc.shape == (0,) and len(ctx.phase_reads()[0]) == 0
    monkeypatch.setenv("VGA_HAP_PATHS_STORE_ROWS", "1")
    ctx.haplotype_paths_begin(cap=64)
    monkeypatch.delenv("VGA_HAP_PATHS_STORE_ROWS")
    bases, edges = [], []
    for part in (seqs[:1], seqs[1:130], seqs[130:]):
        align(ctx, part)
        assert launches(ctx).get("k_hp_keep") == 1
        b_, e_ = ctx.path_support_last()
        bases.append(b_)
        edges.append(e_)
    bases, edges = np.concatenate(bases), np.concatenate(edges)
    d, sc = ctx.haplotype_paths_store()
    assert d.dtype == np.uint8 and d.shape == (300, 12) and np.array_equal(d, sample["deficits"]) and np.array_equal(sc, sample["scored"])
    lik = ctx.genotype_likelihood_pairs(bases, edges, cap=64)
    assert np.array_equal(d, lik["deficit"].reshape(300, 12)) and int(sc.sum()) == lik["n_scored"]
    v = ctx.variant_call()
    het = np.flatnonzero(v["x"] < v["y"])
    pos, x, y = v["pos"][het], v["x"][het], v["y"][het]
    assert pos.tolist() == sample["pos"]
    links, _, _ = ctx.phase_links(pos, x, y)
    ps, flip, _ = p.binding.phase_chain(links)
    assert ps.tolist() == sample["ps"] and flip.tolist() == sample["flip"]
    reads, table, n_sets, n_reads = ctx.haplotype_paths(pos, x, y, ps, flip)
    assert (n_sets, n_reads) == (sample["n_sets"], 300)
    n_k = launches(ctx)
    assert all(n_k.get(k) == 1 for k in KERNELS), n_k
    ref.same(reads, table, sample["reads"], sample["table"], "the context's stores")
    for g, (order, tied) in sample["ranked"].items():
        got_order, got_tied = p.binding.haplotype_paths_rank(table[g])
        assert (got_order.tolist(), got_tied) == (order, tied), g
    monkeypatch.setenv("VGA_PHASE_READ_TILE", "64")
    again = ctx.haplotype_paths(pos, x, y, ps, flip)
    assert launches(ctx).get("k_hp_sums") == 5 and np.array_equal(again[0], reads) and np.array_equal(again[1], table)
    monkeypatch.delenv("VGA_PHASE_READ_TILE")
    recs, words = ctx.phase_reads()
    a = sample["arrays"]
    lists = ctx.haplotype_paths_lists(recs, words, len(a["seq_fwd"]), d, sc, pos, x, y, hc_ref.cref_of(a["seq_fwd"], pos), ps, flip)
    assert np.array_equal(lists[0], reads) and np.array_equal(lists[1], table)
    with pytest.raises(p.VgaError) as e:
        ctx.haplotype_paths(pos, x, y, np.zeros_like(ps), flip)
    assert e.value.code == -1
    # the stores are not reset by the call; phase_reset empties both
    assert len(ctx.haplotype_paths_store()[0]) == 300
    ctx.phase_reset()
    reads, table, n_sets, n_reads = ctx.haplotype_paths(pos, x, y, ps, flip)
    assert reads.shape == (0,) and (n_sets, n_reads) == (0, 0) and len(ctx.haplotype_paths_store()[0]) == 0
    # begin out of order, and the ends
    for bad in (0, 256):
        with pytest.raises(p.VgaError) as e:
            ctx.haplotype_paths_begin(cap=bad)
        assert e.value.code == -1
    with pytest.raises(p.VgaError) as e:
        ctx.haplotype_paths_begin(source="edit")      # the edit distance is off
    assert e.value.code == -1
    ctx.haplotype_paths_end()
    with pytest.raises(p.VgaError):
        ctx.haplotype_paths(pos, x, y, ps, flip)
    ctx.haplotype_paths_begin()
    ctx.phase_end()                                   # drops it
    with pytest.raises(p.VgaError) as e:
        ctx.haplotype_paths_begin()                   # the phase store is off
    assert e.value.code == -1 and "phase" in str(e.value)
    ctx.phase_begin()
    ctx.haplotype_paths_begin()
    ctx.path_support_end()                            # drops it
    with pytest.raises(p.VgaError):
        ctx.haplotype_paths_store()
    with pytest.raises(p.VgaError) as e:
        ctx.haplotype_paths_begin()                   # path support is off
    assert e.value.code == -1 and "path support" in str(e.value)
    align(ctx, seqs[:8])                              # and nothing is kept or launched any more
    assert not any(k.startswith("k_hp") for k in launches(ctx)), launches(ctx)
    ctx.phase_end()
    ctx.pileup_end()


def test_cli(drb1, sample, tmp_path):
    d = str(tmp_path)
    a = sample["arrays"]
    fa, fa_few = os.path.join(d, "r.fa"), os.path.join(d, "few.fa")
    few = sample["sim"][:60]
    for name, reads in ((fa, sample["sim"]), (fa_few, few)):
        with open(name, "w") as f:
            for r in reads:
                f.write(">%s\n%s\n" % (r.name, r.seq))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1, "--call-variants", "--phase"]
    extra = ["--haplotag", "--haplotype-calls"]
    pr = run(common + ["-o", os.path.join(d, "plain")] + extra)
    assert "haplotype-paths" not in pr.stderr and not [f for f in os.listdir(d) if "-haplotype-paths" in f]
    read = lambda name: open(os.path.join(d, name)).read()
    assert read("plain-alignments.gaf") == sample["gaf"]
    assert sample["tsv"].count("\n") > 1 + 5 * 4
    for out, more in (("one", []), ("chunks", ["--chunk-reads", "8"]), ("two", ["--devices", "0,0", "--chunk-reads", "8"])):
        pr = run(common + ["-o", os.path.join(d, out), "--haplotype-paths"] + extra + more)
        assert read(out + "-haplotype-paths.tsv") == sample["tsv"], out
        for line in sample["stderr"]:
            assert "[vgaligner] " + line + "\n" in pr.stderr, (line, pr.stderr)
        # every other file is byte for byte what it is without the switch; path support writes no file of its own
        files = {f[len(out):] for f in os.listdir(d) if f.startswith(out + "-")}
        assert files == {f[len("plain"):] for f in os.listdir(d) if f.startswith("plain-")} | {"-haplotype-paths.tsv"}
        for suffix in files - {"-haplotype-paths.tsv"}:
            assert read(out + suffix) == read("plain" + suffix), (out, suffix)
        assert "-phase.tsv" in files and "-haplotag.tsv" in files and "-path-support.tsv" not in files
    # the switch alone, all paths, another cap
    other = ref.gaf(sample["gaf"], DRB1, a["node_seq_idx"], a["seq_fwd"], cap=3, top=0)
    pr = run(common + ["-o", os.path.join(d, "cap"), "--haplotype-paths", "--haplotype-paths-cap", "3", "--haplotype-paths-top", "0"])
    assert read("cap-haplotype-paths.tsv") == other["tsv"] != sample["tsv"] and other["stderr"][1] in pr.stderr
    assert not os.path.exists(os.path.join(d, "cap-haplotag.tsv")) and read("cap-phase.tsv") == read("plain-phase.tsv")
    # under --phase-join the file follows the joined sets
    joined = ref.gaf(sample["gaf"], DRB1, a["node_seq_idx"], a["seq_fwd"], join=True)
    assert joined["ps"] != sample["ps"] and joined["tsv"] != sample["tsv"]
    pr = run(common + ["-o", os.path.join(d, "join"), "--haplotype-paths", "--phase-join", "--devices", "0,0", "--chunk-reads", "64"])
    assert read("join-haplotype-paths.tsv") == joined["tsv"] and all(line in pr.stderr for line in joined["stderr"])
    # from the edit distance, on the first 60 reads (the reference's edit distance is slow)
    few_gaf = "".join(line + "\n" for line in sample["gaf"].splitlines()[:len(few)])
    edit = ref.gaf(few_gaf, DRB1, a["node_seq_idx"], a["seq_fwd"], read_seqs=[r.seq for r in few], source="edit", min_depth=2)
    support = ref.gaf(few_gaf, DRB1, a["node_seq_idx"], a["seq_fwd"], min_depth=2)
    assert edit["n_sets"] > 0 and len(edit["ranked"]) > 0 and edit["tsv"] != support["tsv"]
    common_few = [fa_few if v == fa else v for v in common] + ["--call-min-depth", "2"]
    pr = run(common_few + ["-o", os.path.join(d, "edit"), "--haplotype-paths", "--haplotype-paths-from", "edit"])
    assert read("edit-haplotype-paths.tsv") == edit["tsv"] and all(line in pr.stderr for line in edit["stderr"])
    assert not os.path.exists(os.path.join(d, "edit-path-edit.tsv"))
    pr = run(common_few + ["-o", os.path.join(d, "support"), "--haplotype-paths", "--devices", "0,0", "--chunk-reads", "16"])
    assert read("support-haplotype-paths.tsv") == support["tsv"]
    # no heterozygous site: the header only
    pr = run(common + ["-o", os.path.join(d, "none"), "--haplotype-paths", "--call-min-depth", "1000"])
    assert read("none-haplotype-paths.tsv") == ref.HEADER + "\n" and "haplotype-paths: no call" in pr.stderr
    assert "haplotype-paths: 0 sets, 0 groups with reads, %d of 300 kept reads scored" % int(sample["scored"].sum()) in pr.stderr
