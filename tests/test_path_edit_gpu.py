"""The edit distance of reads to haplotype paths on the GPU (vga_path_edit_begin / _read / _last / _reset / _end / _pairs,
vga_genotype_lik_source, k_pe_jobs, k_pe_dist, k_pe_rows, `vgaligner map --path-edit`).  Every comparison is exact equality of
integers with tests/path_edit_ref.py: through the kernel seam over explicit strings, and end to end over the ORACLE's alignments GAF,
the GFA and the reads.  Without the feature every test here stops at Context.path_edit_pairs / path_edit_begin (no such call) or at
the unknown --path-edit flag."""
import os
import random
import subprocess

import numpy as np
import pytest

import genotype_lik_ref
import path_edit_ref as ref
import path_support_ref
from helpers import DATA, ROOT, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
A3105 = os.path.join(DATA, "hla", "4-A3105.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
NONE = ref.NONE
LAM, CAP = 512, 64
KERNELS = ["k_pe_jobs", "k_pe_dist", "k_pe_rows"]


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


def rnd(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def mutate(rng, s, rate, alphabet="ACGT"):
    out = []
    for c in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out.append(rng.choice(alphabet))
            continue
        if x < rate:
            out.append(c)
            out.append(rng.choice(alphabet))
            continue
        out.append(c)
    return "".join(out)


def planted(rng, m, n, alphabet="ACGT", rate=0.1):
    """a query of m letters and a text of n that holds a copy of it with `rate` edits where there is room, else random letters"""
    q = rnd(rng, m, alphabet)
    t = rnd(rng, n, alphabet)
    if n > m + 10:
        at = rng.randrange(0, n - m)
        t = (t[:at] + mutate(rng, q, rate, alphabet) + t[at + m:] + rnd(rng, m, alphabet))[:n]
    assert len(t) == n
    return q, t


def check(ctx, pairs, what):
    """the pairs through the seam in ONE call against the Myers reference, a few of them against the column DP as well"""
    got = ctx.path_edit_pairs([q for q, _ in pairs], [t for _, t in pairs])
    limit = pkg().binding.PATH_EDIT_MAX_QUERY
    want = [NONE if len(q) > limit else ref.myers_distance(q, t) for q, t in pairs]
    assert got.dtype == np.uint32 and got.tolist() == want, (what, [(i, len(pairs[i][0]), len(pairs[i][1]), int(got[i]), want[i])
                                                                    for i in range(len(pairs)) if int(got[i]) != want[i]][:8])
    return got


# =====================================================================================================================
# 1. the kernel seam
# =====================================================================================================================
def test_seam_reference_distances_agree_on_these_shapes():
    rng = random.Random(3)
    for m, n in ((1, 1), (63, 65), (65, 300), (129, 64), (200, 700)):
        q, t = planted(rng, m, n, "ACGTNacgt")
        assert ref.myers_distance(q, t) == ref.dp_distance(q, t), (m, n)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 127, 128, 129])
def test_seam_block_edges(ctx, m):
    """one block that is not full, full, one row into the next (and the same for two blocks), against texts of one column, one short
    of, exactly and one past the 64-column fetch, texts that are no multiple of it, and texts shorter than the lanes in use"""
    rng = random.Random(100 + m)
    pairs = [planted(rng, m, n) for n in (1, 2, 63, 64, 65, 127, 129, 200, 333) for _ in range(2)]
    check(ctx, pairs, "m %d" % m)
    assert [t["name"] for t in ctx.kernel_times()] == ["k_pe_encode", "k_pe_dist"]


def r_edges():
    b = pkg().binding
    out, R = [], 1
    while R <= b.PATH_EDIT_MAX_R:
        out.append((R, 64 * R * 64))
        R *= 2
    return out


@pytest.mark.parametrize("R,full", r_edges())
def test_seam_switch_to_the_next_blocks_per_lane_and_the_last_lane(ctx, R, full):
    """m = 64 R 64 - 1, exactly that and + 1: the last row of the last lane's last block, and the first query served with the next R
    (past the largest R: skipped, NONE, not an error).  Texts: a planted copy with 10 % edits, a text shorter than the lanes in use
    (the pipeline drains with columns in flight), one column, and a text that is no multiple of the fetch"""
    b = pkg().binding
    rng = random.Random(full)
    pairs = []
    for m in (full - 1, full, full + 1):
        pairs.append(planted(rng, m, m + 517))
        pairs.append(planted(rng, m, 37))
        pairs.append(planted(rng, m, 1))
        q = rnd(rng, m)
        pairs.append((q, "C" * 70 + q))   # the optimum ends at the last column
    got = check(ctx, pairs, "R %d" % R)
    if full == b.PATH_EDIT_MAX_QUERY:
        assert got[8:].tolist() == [NONE] * 4 and NONE not in got[:8].tolist()
        assert got[7] == 0
    else:
        assert NONE not in got.tolist() and got[11] == 0


def test_seam_contents(ctx):
    rng = random.Random(9)
    q300 = rnd(rng, 300)
    q70 = rnd(rng, 70, "ACGTNacgtn")
    pairs = [
        (q300, q300),                                   # identical strings
        ("A" * 150, "C" * 400),                         # nothing matches: e = m
        ("N" * 100, "N" * 100),                         # N matches nothing, not even N
        ("G" * 99 + "A", "A" + "C" * 300),              # the optimum ends at the first column: e = m - 1
        (q300, "C" * 333 + q300),                       # ... at the last column: e = 0
        ("ACGT" * 20, "TTTT" * 50),                     # e < m only through single letters
        (q300, q300[100:150]),                          # m > n: e = 250
        (q70, q70.swapcase()),                          # lower case equals upper case; N equals nothing
        (q70.lower(), mutate(rng, q70.upper() * 3, 0.1, "ACGTN")),
        ("acgtRYKM" * 10, "ACGTRYKM" * 12),             # other letters match nothing on either side
        ("", "ACGT"),                                   # an empty query: 0
        ("ACGT", ""),                                   # an empty text: m
    ]
    got = check(ctx, pairs, "contents")
    assert got[0] == 0 and got[1] == 150 and got[2] == 100 and got[3] == 99 and got[4] == 0 and got[6] == 250
    assert 0 < got[7] <= sum(c in "Nn" for c in q70) and got[10] == 0 and got[11] == 4
    for q, t in pairs[:4] + pairs[5:]:
        assert ref.dp_distance(q, t) == ref.myers_distance(q, t)


def test_seam_random_edits_and_many_jobs_of_mixed_r_in_one_call(ctx):
    """300 jobs whose queries are served with R = 1, 2 and 4 (and one past the limit) in one call, 10 % random edits, N among the
    letters"""
    rng = random.Random(77)
    pairs = [planted(rng, rng.randrange(1, 400), rng.randrange(1, 900), "ACGTN") for _ in range(290)]
    for m in (4097, 5000, 8193, 9000, 16000, 16385, 4096, 700, 8192, 64):
        pairs.append(planted(rng, m, m + rng.randrange(11, 300)))
    rng.shuffle(pairs)
    b = pkg().binding
    assert {b.PATH_EDIT_MAX_QUERY // 4 < len(q) for q, _ in pairs} == {True, False}
    got = check(ctx, pairs, "mixed")
    assert got.tolist().count(NONE) == 1


def test_seam_refuses_bad_arguments(ctx):
    p = pkg()
    L = p.binding.load_library()
    u64 = p.binding._u64p
    out = np.zeros(2, dtype=np.uint32)
    off = np.array([0, 4], dtype=np.uint64)
    down = np.array([4, 0], dtype=np.uint64)
    assert L.vga_path_edit_pairs(ctx.h, 0, None, None, None, None, None) == 0
    assert L.vga_path_edit_pairs(ctx.h, 1, None, b"ACGT", u64(off), b"ACGT", p.binding._u32p(out)) == -1
    assert L.vga_path_edit_pairs(ctx.h, 1, u64(off), b"ACGT", u64(off), b"ACGT", None) == -1
    assert L.vga_path_edit_pairs(ctx.h, 1, u64(down), b"ACGT", u64(off), b"ACGT", p.binding._u32p(out)) == -1
    assert L.vga_path_edit_pairs(ctx.h, 1, u64(off), None, u64(off), b"ACGT", p.binding._u32p(out)) == -1
    assert L.vga_path_edit_pairs(ctx.h, 1, u64(off), b"ACGT", u64(off), b"ACGA", p.binding._u32p(out)) == 0 and out[0] == 1
    assert ctx.path_edit_pairs([], []).shape == (0,)


# =====================================================================================================================
# 2. end to end: the matrix and the accumulators against the reference over the oracle's GAF
# =====================================================================================================================
def walker(oracle, ix, seqs):
    _, ag, _ = oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, oracle.default_map_params())
    return ref.walk(ag, seqs, DRB1), ag


def fresh(c, ix, gfa=DRB1):
    upload_oracle_index(c, ix)
    g = pkg().hostlib.gfa_paths(gfa)
    c.path_support_begin(g["step_off"], g["steps"])
    c.path_edit_begin()


def score(c, seqs, map_params=None):
    b = c.batch(seqs)
    mo = b.map(map_params) if map_params is not None else b.map()
    al = b.align(mo, best_n=1)
    b.close()
    return al, mo


def same_matrix(got, w, what):
    assert got.dtype == np.uint32 and got.shape == w["edit"].shape, (what, got.shape)
    bad = np.argwhere(got.astype(np.int64) != w["edit"])
    assert len(bad) == 0, (what, len(bad), [(r, p, int(got[r, p]), int(w["edit"][r, p])) for r, p in bad[:6].tolist()])


@pytest.fixture(scope="module")
def drb1_case(oracle, drb1):
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)]
    w, ag = walker(oracle, drb1, seqs)
    assert w["n_alignments"] == len(seqs) and w["n_too_long"] == 0
    # path 6 of DRB1 has only "id-" steps: a whole NONE column, which must not disturb the row minima
    assert (w["edit"][:, 6] == NONE).all() and w["n_scored"][6] == 0 and w["best"][6] == 0
    assert (w["edit"][:, [p for p in range(12) if p != 6]] != NONE).any()
    assert w["best"].sum() >= len(seqs) and 0 < w["best_alone"].sum()
    return seqs, w, ag


@pytest.fixture(scope="module")
def second_case(oracle, drb1):
    s2 = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 7, 1500, 0.03, 0.03, 0.04, seed=52)] + ["ACGT" * 30]
    w2, _ = walker(oracle, drb1, s2)
    assert w2["n_alignments"] == 7 and (w2["edit"][7] == NONE).all()  # (the last read has no chain: a placeholder record, a NONE row)
    return s2, w2


def test_drb1(ctx, drb1, drb1_case):
    seqs, w, _ = drb1_case
    fresh(ctx, drb1)
    score(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_ps_score" in names and all(k in names for k in KERNELS) and "k_gl_pairs" not in names, names
    same_matrix(ctx.path_edit_last(), w, "DRB1 k=11")
    ref.same(ctx.path_edit(), w, "DRB1 k=11")
    ref.same(ctx.path_edit(), w, "read twice")
    # the matrix through the seam: the same distance kernel over the windows the reference cuts
    wins, pseqs = ref.windows(drb1_case[2], seqs, DRB1)
    jobs = [(r, p, q, pseqs[p][lh[0]:lh[1]]) for r, (q, per) in enumerate(wins) for p, lh in enumerate(per) if lh is not None][::7]
    got = ctx.path_edit_pairs([j[2] for j in jobs], [j[3] for j in jobs])
    assert got.tolist() == [int(w["edit"][r, p]) for r, p, _, _ in jobs]
    ref.same(ctx.path_edit(), w, "the seam leaves the accumulators alone")
    # path support itself is what it is without the edit distance
    node_len, paths = path_support_ref.parse_gfa(DRB1)
    ws = path_support_ref.walk(drb1_case[2], node_len, paths)
    b, e = ctx.path_support_last()
    assert np.array_equal(b, ws["bases"]) and np.array_equal(e, ws["edges"])
    ctx.path_support_end()


def test_two_batches_and_reset(ctx, drb1, drb1_case, second_case):
    seqs, w, _ = drb1_case
    s2, w2 = second_case
    fresh(ctx, drb1)
    score(ctx, seqs)
    score(ctx, s2)
    same_matrix(ctx.path_edit_last(), w2, "the second batch")
    ref.same(ctx.path_edit(), ref.add(w, w2), "two batches")
    ctx.path_edit_reset()
    got = ctx.path_edit()
    assert not any(got[k].any() for k in ref.FIELDS) and got["n_alignments"] == 0 and got["n_too_long"] == 0
    score(ctx, s2)
    ref.same(ctx.path_edit(), w2, "after reset")
    ctx.path_support_end()


def test_both_strands(oracle, ctx, drb1):
    p = pkg()
    reads = p.readsim.simulate_reads(DRB1, 24, 2500, 0.03, 0.03, 0.04, seed=31, reverse_fraction=0.5)
    seqs = [r.seq for r in reads]
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    fresh(ctx, drb1)
    al, mo = score(ctx, seqs, map_params=mp)
    assert 0 < int(mo.strand.sum()) < len(seqs)
    chosen = [p.readsim.reverse_complement(s) if st else s for s, st in zip(seqs, mo.strand.tolist())]
    w, _ = walker(oracle, drb1, chosen)
    same_matrix(ctx.path_edit_last(), w, "both strands")
    ref.same(ctx.path_edit(), w, "both strands")
    ctx.path_support_end()


def test_a_read_past_the_limit_is_skipped_and_counted(oracle, ctx):
    """a read of 16 385 letters that aligns: a NONE row, counted in n_too_long and in n_alignments, beside a read that is scored.  The
    node paths come from the call's own records."""
    p = pkg()
    node_seq, paths = ref.parse_gfa(A3105)
    longest = max(range(len(paths)), key=lambda i: sum(len(node_seq[n]) for n, _ in paths[i][1]))
    seq, _ = ref.path_sequence(paths[longest][1], node_seq)
    limit = p.binding.PATH_EDIT_MAX_QUERY
    seqs = [seq[2000:2000 + limit + 1].upper(), seq[30000:32000].upper()]
    assert len(seqs[0]) == limit + 1
    ix = oracle.Index(oracle.Graph.from_gfa(A3105), 11)
    fresh(ctx, ix, A3105)
    al, _ = score(ctx, seqs)
    assert al.aligned.tolist() == [1, 1]
    lines = []
    for r in range(2):
        hs = al.path_handles[int(al.path_off[r]):int(al.path_off[r + 1])].tolist()
        assert not any(h & 1 for h in hs)
        lines.append("\t".join(["r%d" % r, "0", "0", "0", "+", "".join(">%d" % (h >> 1) for h in hs)] + ["0"] * 6))
    w = ref.walk("\n".join(lines) + "\n", seqs, A3105)
    assert w["n_too_long"] == 1 and w["n_alignments"] == 2 and (w["edit"][0] == NONE).all() and (w["edit"][1] != NONE).any()
    same_matrix(ctx.path_edit_last(), w, "past the limit")
    ref.same(ctx.path_edit(), w, "past the limit")
    ctx.path_support_end()


# =====================================================================================================================
# 3. the likelihood from the edit distance
# =====================================================================================================================
def test_genotype_likelihood_from_edit_and_from_support(ctx, drb1, drb1_case, second_case):
    seqs, w, ag = drb1_case
    s2, w2 = second_case
    T = pkg().binding.genotype_likelihood_table(LAM, CAP)
    want = genotype_lik_ref.pairs(*ref.likelihood_matrices(w), LAM, CAP, T)
    want2 = genotype_lik_ref.pairs(*ref.likelihood_matrices(w2), LAM, CAP, T)
    assert want["n_scored"] == len(seqs) and want2["n_scored"] == 7
    fresh(ctx, drb1)
    ctx.genotype_likelihood_begin(LAM, CAP, source="edit")
    score(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert all(k in names for k in KERNELS + ["k_gl_deficit", "k_gl_pairs"]), names
    genotype_lik_ref.same(ctx.genotype_likelihood(), want, "from edit", deficit=False)
    ref.same(ctx.path_edit(), w, "the accumulators beside the likelihood")
    score(ctx, s2)  # (a placeholder row: all NONE, costs nothing)
    genotype_lik_ref.same(ctx.genotype_likelihood(), genotype_lik_ref.add(want, want2), "two batches from edit", deficit=False)
    # from support it is what it is today, with the edit distance on beside it
    node_len, paths = path_support_ref.parse_gfa(DRB1)
    ws = path_support_ref.walk(ag, node_len, paths)
    ctx.genotype_likelihood_begin(LAM, CAP, source="support")
    score(ctx, seqs)
    genotype_lik_ref.same(ctx.genotype_likelihood(), genotype_lik_ref.pairs(ws["bases"], ws["edges"], LAM, CAP, T), "from support", deficit=False)
    same_matrix(ctx.path_edit_last(), w, "beside the likelihood from support")
    # the source needs both features on
    p = pkg()
    ctx.path_edit_end()
    with pytest.raises(p.VgaError) as e:
        ctx.genotype_likelihood_begin(LAM, CAP, source="edit")
    assert e.value.code == -1 and "vga_path_edit_begin" in str(e.value)
    with pytest.raises(p.VgaError):
        ctx.genotype_likelihood()  # (the refused begin leaves the likelihood off)
    with pytest.raises(p.VgaError):
        ctx.genotype_likelihood_begin(LAM, CAP, source="bases")
    L = p.binding.load_library()
    ctx.genotype_likelihood_begin(LAM, CAP)
    assert L.vga_genotype_lik_source(ctx.h, 2) == -1 and L.vga_genotype_lik_source(ctx.h, p.binding.VGA_GL_FROM_SUPPORT) == 0
    ctx.genotype_likelihood_end()
    assert L.vga_genotype_lik_source(ctx.h, 0) == -1
    ctx.path_support_end()


# =====================================================================================================================
# 4. life cycle, and the feature off
# =====================================================================================================================
def test_life_cycle_and_feature_off(drb1, drb1_case):
    p = pkg()
    seqs, w, _ = drb1_case
    seqs = seqs[:6]
    g = p.hostlib.gfa_paths(DRB1)
    c = p.Context(0)
    pe_names = lambda: [t["name"] for t in c.kernel_times() if t["name"].startswith("k_pe")]

    def refused(call, what):
        with pytest.raises(p.VgaError) as e:
            call()
        assert e.value.code == -1, what

    try:
        refused(c.path_edit_begin, "begin without an index")
        upload_oracle_index(c, drb1)
        refused(c.path_edit_begin, "begin without path support")
        assert "path support" in p.binding.load_library().vga_last_error(c.h).decode()
        refused(c.path_edit, "read before begin")
        refused(c.path_edit_reset, "reset before begin")
        c.path_edit_end()  # (ending what is off is harmless)
        c.path_support_begin(g["step_off"], g["steps"])
        refused(lambda: c.path_edit_last(6), "last while it is off")
        al0, _ = score(c, seqs)
        assert pe_names() == [], "off: no launch"
        c.path_edit_begin()
        assert pe_names() == ["k_pe_paths"]
        refused(lambda: c.path_edit_last(6), "last before any batch")
        al1, _ = score(c, seqs)
        assert pe_names() == KERNELS
        assert al1.cs == al0.cs and al1.cigar == al0.cigar and np.array_equal(al1.path_handles, al0.path_handles)
        assert np.array_equal(c.path_edit_last().astype(np.int64), w["edit"][:6])
        refused(lambda: c.path_edit_last(5), "last with another batch's size")
        c.path_edit_end()
        score(c, seqs)
        assert pe_names() == [] and c.path_support()["n_alignments"] == 18, "path support goes on"
        # path_support_end, a second path_support_begin and a new index end it
        c.path_edit_begin()
        c.path_support_begin(g["step_off"], g["steps"])
        refused(c.path_edit, "read after a second path_support_begin")
        c.path_edit_begin()
        c.path_support_end()
        refused(c.path_edit, "read after path_support_end")
        c.path_support_begin(g["step_off"], g["steps"])
        c.path_edit_begin()
        upload_oracle_index(c, drb1)
        refused(c.path_edit, "read after a new index")
        score(c, seqs)
        assert not any(t["name"].startswith(("k_ps", "k_pe")) for t in c.kernel_times())
    finally:
        c.close()


# =====================================================================================================================
# 5. the executable
# =====================================================================================================================
def test_cli(oracle, drb1, tmp_path):
    p = pkg()
    d = str(tmp_path)
    reads = p.readsim.config3_reads(DRB1, 24, 3000)
    fa = os.path.join(d, "r.fa")
    with open(fa, "w") as f:
        for r in reads:
            f.write(">%s\n%s\n" % (r.name, r.seq))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    seqs = [r.seq for r in reads]
    ocg, oag, _ = oracle.map_reads(drb1, [r.name for r in reads], seqs)
    w = ref.walk(oag, seqs, DRB1)
    node_seq, paths = ref.parse_gfa(DRB1)
    per_path = "path\tsteps\tlength\tscored\tsum_edit\tbest\tbest_alone\n" + "".join(
        "%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, len(st), sum(len(node_seq[n]) for n, _ in st), w["n_scored"][i], w["sum_edit"][i], w["best"][i], w["best_alone"][i])
        for i, (name, st) in enumerate(paths))
    per_read = "read\tpath\tedit\n" + "".join("%d\t%d\t%d\n" % (r, q, w["edit"][r, q]) for r in range(len(seqs)) for q in range(12) if w["edit"][r, q] != NONE)
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain")])
    line = "path-edit: %d alignments, 12 paths, 0 too long" % w["n_alignments"]
    for out, extra in (("one", ["--path-edit"]), ("two", ["--path-edit", "--devices", "0,0", "--chunk-reads", "10"]),
                       ("three", ["--path-edit", "--path-support", "--genotype", "--coverage", "--pileup", "--genotype-likelihood", "--genotype-from", "support"])):
        pr = run(common + ["-o", os.path.join(d, out)] + extra)
        pre = os.path.join(d, out)
        assert line in pr.stderr, (line, pr.stderr)
        assert open(pre + "-path-edit.tsv").read() == per_path, out
        assert open(pre + "-path-edit-reads.tsv").read() == per_read, out
        assert open(pre + "-chains.gaf").read() == open(os.path.join(d, "plain-chains.gaf")).read() == ocg, out
        assert open(pre + "-alignments.gaf").read() == open(os.path.join(d, "plain-alignments.gaf")).read() == oag, out
    assert not os.path.exists(os.path.join(d, "plain-path-edit.tsv")) and not os.path.exists(os.path.join(d, "plain-path-edit-reads.tsv"))
    # --genotype-from support: the table path support's matrices give; --genotype-from edit: the table of the reference's m - e, and
    # no path-edit file without --path-edit
    T = p.binding.genotype_likelihood_table(LAM, CAP)
    names = [name for name, _ in paths]

    def table_text(bases, edges):
        ranked = genotype_lik_ref.rank(genotype_lik_ref.pairs(bases, edges, LAM, CAP, T)["cost"], 12, 20)
        return "rank\tpath_a\tpath_b\tcost\tmargin\n" + "".join("%d\t%s\t%s\t%d\t%d\n" % (i + 1, names[a], names[b], c, m) for i, (a, b, c, m) in enumerate(ranked))

    ws = path_support_ref.walk(oag, *path_support_ref.parse_gfa(DRB1))
    assert open(os.path.join(d, "three-genotype-likelihood.tsv")).read() == table_text(ws["bases"], ws["edges"])
    run(common + ["-o", os.path.join(d, "ed"), "--genotype-likelihood", "--genotype-from", "edit"])
    assert open(os.path.join(d, "ed-genotype-likelihood.tsv")).read() == table_text(*ref.likelihood_matrices(w))
    assert open(os.path.join(d, "ed-genotype-likelihood.tsv")).read() != open(os.path.join(d, "three-genotype-likelihood.tsv")).read()
    assert not os.path.exists(os.path.join(d, "ed-path-edit.tsv")) and not os.path.exists(os.path.join(d, "ed-path-edit-reads.tsv"))
    # --both-strands: the table of that run's own records, '-' ones among them
    run(common + ["-o", os.path.join(d, "four"), "--both-strands", "--path-edit"])
    wb = ref.walk(open(os.path.join(d, "four-alignments.gaf")).read(), seqs, DRB1)
    assert open(os.path.join(d, "four-path-edit-reads.tsv")).read() == "read\tpath\tedit\n" + "".join(
        "%d\t%d\t%d\n" % (r, q, wb["edit"][r, q]) for r in range(len(seqs)) for q in range(12) if wb["edit"][r, q] != NONE)
