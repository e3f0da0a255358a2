"""The variant call on the GPU (vga_variant_call / vga_variant_call_table, k_vc_count + k_vc_scan + k_vc_emit, `vgaligner map
--call-variants`).  Every comparison is exact equality with the plain reference (tests/variant_ref.py): through the kernel seam at
the sizes where the compaction and the costs can go wrong, through a context against the reference applied to that context's own
pileup table and to the oracle's alignments GAF, and through the executable.  Without the feature every test here stops at a
missing symbol or at the unknown --call-variants flag."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pileup_ref
import variant_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
WG = 256  # bases of a workgroup of k_vc_count / k_vc_emit
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


def random_table(n, seed, top=8, letters="ACGTacgtN"):
    rng = np.random.default_rng(seed)
    return rng.integers(0, top + 1, size=(n, 7)).astype(np.uint64), "".join(rng.choice(list(letters), size=n))


def clean_table(n, seed, depth=8):
    """every base read `depth` times as its own letter: nothing to report"""
    rng = np.random.default_rng(seed)
    letters = "".join(rng.choice(list("ACGT"), size=n))
    tab = np.zeros((n, 7), dtype=np.uint64)
    tab[np.arange(n), [pileup_ref.column(c) for c in letters]] = depth
    return tab, letters


def agree(got, want, what=""):
    print(what, "tested", got["n_tested"], "/", want["n_tested"], "calls", got["n_calls"], "/", want["n_calls"])
    bad = variant_ref.same(got, want)
    assert bad is None, (what, bad, np.asarray(got[bad]).tolist()[:8], np.asarray(want[bad]).tolist()[:8])


def raw_table(c, tab, letters, cap, error=1280, min_depth=4, min_qual=512, room=None):
    """vga_variant_call_table with a cap of the caller's choice (the wrapper would ask again) into arrays filled with a sentinel:
    -> (return code, n_tested, n_calls, the arrays)"""
    L = pkg().binding.load_library()
    tab = np.ascontiguousarray(tab, dtype=np.uint64)
    room = max(1, cap if room is None else room)
    arr = {"pos": np.full(room, SENTINEL, dtype=np.uint32), "gt": np.full(room, SENTINEL, dtype=np.uint8), "qual": np.full(room, SENTINEL, dtype=np.uint32),
           "ins_qual": np.full(room, SENTINEL, dtype=np.uint64), "depth": np.full(room, SENTINEL, dtype=np.uint64),
           "counts": np.full((room, 7), SENTINEL, dtype=np.uint64)}
    nt, nc = C.c_uint64(SENTINEL), C.c_uint64(SENTINEL)
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    rc = L.vga_variant_call_table(c.h, len(tab), p(tab, C.c_uint64), letters.encode(), error, min_depth, min_qual, cap, p(arr["pos"], C.c_uint32),
                                  p(arr["gt"], C.c_uint8), p(arr["qual"], C.c_uint32), p(arr["ins_qual"], C.c_uint64), p(arr["depth"], C.c_uint64),
                                  p(arr["counts"], C.c_uint64), C.byref(nt), C.byref(nc))
    return rc, int(nt.value), int(nc.value), arr


# ---- 1. the seam: sizes around a wave and a workgroup
@pytest.mark.parametrize("n", [1, 63, 64, 65, WG - 1, WG, WG + 1])
def test_seam_sizes(ctx, n):
    tab, letters = random_table(n, seed=100 + n)
    want = variant_ref.call_table(tab, letters)
    assert n == 1 or 0 < want["n_calls"] < n
    agree(ctx.variant_call_table(tab, letters), want, "n=%d" % n)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_vc_count" in names and "k_vc_scan" in names, names


def test_one_base_that_is_a_call_and_one_that_is_not(ctx):
    got = ctx.variant_call_table([[0, 0, 9, 0, 0, 0, 0]], "A")
    agree(got, variant_ref.call_table([[0, 0, 9, 0, 0, 0, 0]], "A"))
    assert got["n_calls"] == 1 and (int(got["x"][0]), int(got["y"][0]), int(got["pos"][0])) == (2, 2, 0)
    got = ctx.variant_call_table([[9, 0, 0, 0, 0, 0, 0]], "A")
    assert (got["n_tested"], got["n_calls"]) == (1, 0) and len(got["pos"]) == 0
    got = ctx.variant_call_table(np.zeros((0, 7), dtype=np.uint64), "")
    assert (got["n_tested"], got["n_calls"]) == (0, 0)


@pytest.mark.parametrize("n,edge", [(3 * WG + 17, WG), (3 * WG + 17, 2 * WG), (5 * WG, 4 * WG), (5 * WG, 3 * WG)])
def test_only_calls_on_the_edge_of_two_workgroups(ctx, n, edge):
    """the last lane of one workgroup and the first lane of the next, in a table that reports nothing else"""
    tab, letters = clean_table(n, seed=n + edge)
    for i, alt in ((edge - 1, "del"), (edge, "sub")):
        r = pileup_ref.column(letters[i])
        tab[i] = 0
        tab[i, 5 if alt == "del" else (r + 1) % 4] = 8
    want = variant_ref.call_table(tab, letters)
    assert want["pos"].tolist() == [edge - 1, edge] and want["n_tested"] == n
    agree(ctx.variant_call_table(tab, letters), want, "edge %d of %d" % (edge, n))


def test_no_call_writes_nothing(ctx):
    tab, letters = clean_table(3 * WG + 5, seed=3)
    rc, nt, nc, arr = raw_table(ctx, tab, letters, cap=16)
    assert (rc, nt, nc) == (0, len(tab), 0)
    for a in arr.values():
        assert (a == SENTINEL).all()
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_vc_emit" not in names, names  # nothing to place: the third kernel is not launched


def test_every_base_a_call(ctx):
    n = 4 * WG + 3
    tab, letters = clean_table(n, seed=4)
    own = np.array([pileup_ref.column(c) for c in letters])
    tab[:] = 0
    tab[np.arange(n), (own + 1) % 4] = 5 + (np.arange(n) % 7).astype(np.uint64)   # the depth tells the rows apart
    want = variant_ref.call_table(tab, letters)
    assert want["n_calls"] == n and want["pos"].tolist() == list(range(n))
    agree(ctx.variant_call_table(tab, letters), want, "every base")


@pytest.mark.parametrize("cap", [0, 1, 63, WG + 1])
def test_cap_below_the_calls(ctx, cap):
    """the first cap calls and the true total; nothing behind cap is touched"""
    tab, letters = random_table(4 * WG + 9, seed=5)
    want = variant_ref.call_table(tab, letters)
    assert want["n_calls"] > WG + 1
    rc, nt, nc, arr = raw_table(ctx, tab, letters, cap=cap, room=cap + 8)
    assert (rc, nt, nc) == (0, want["n_tested"], want["n_calls"])
    assert arr["pos"][:cap].tolist() == want["pos"][:cap].tolist()
    assert (arr["gt"][:cap] & 7).tolist() == want["x"][:cap].tolist() and ((arr["gt"][:cap] >> 3) & 7).tolist() == want["y"][:cap].tolist()
    assert (arr["gt"][:cap] >> 6).tolist() == want["ins"][:cap].tolist()
    assert arr["qual"][:cap].tolist() == want["qual"][:cap].tolist() and arr["ins_qual"][:cap].tolist() == want["ins_qual"][:cap].tolist()
    assert arr["depth"][:cap].tolist() == want["depth"][:cap].tolist() and arr["counts"][:cap].tolist() == want["counts"][:cap].tolist()
    for a in arr.values():
        assert (a[cap:] == SENTINEL).all()
    if cap == 0:  # ... and the arrays may be missing altogether
        L = pkg().binding.load_library()
        t = np.ascontiguousarray(tab)
        nt2, nc2 = C.c_uint64(0), C.c_uint64(0)
        assert L.vga_variant_call_table(ctx.h, len(t), t.ctypes.data_as(C.POINTER(C.c_uint64)), letters.encode(), 1280, 4, 512, 0, None, None, None, None, None,
                                        None, C.byref(nt2), C.byref(nc2)) == 0
        assert (nt2.value, nc2.value) == (want["n_tested"], want["n_calls"])
    # the wrapper asks again and gets them all
    agree(ctx.variant_call_table(tab, letters, cap=cap), want, "cap %d, asked again" % cap)


def test_counters_at_the_top_of_32_bits(ctx):
    m = 2**32 - 1
    n = WG + 44
    letters = ("ACGTNacgtn" * n)[:n]
    tab = np.full((n, 7), m, dtype=np.uint64)
    want = variant_ref.call_table(tab, letters, error=8192)
    assert want["n_calls"] == want["n_tested"] > 0 and int(want["depth"][0]) == 6 * m   # (the insertion state is het everywhere)
    agree(ctx.variant_call_table(tab, letters, error=8192), want, "2^32 - 1 everywhere")
    # ... and one column at a time
    tab = np.zeros((7 * 4, 7), dtype=np.uint64)
    for i in range(len(tab)):
        tab[i, i % 7] = m
    letters = ("AAAAAAACCCCCCCGGGGGGGTTTTTTT")
    agree(ctx.variant_call_table(tab, letters, error=8192), variant_ref.call_table(tab, letters, error=8192), "one column at 2^32 - 1")


def test_counters_just_below_2_40_and_the_refusal_at_2_40(ctx):
    p = pkg()
    top = 2**40 - 1
    tab, letters = random_table(2 * WG + 31, seed=6)
    rng = np.random.default_rng(7)
    tab[rng.random(tab.shape) < 0.3] = top
    tab[-1] = top
    for error in (257, 8192):
        want = variant_ref.call_table(tab, letters, error=error)
        assert int(want["qual"].max()) == variant_ref.QUAL_MAX and int(want["ins_qual"].max()) > 2**40
        agree(ctx.variant_call_table(tab, letters, error=error), want, "below 2^40, E=%d" % error)
    for where in ((0, 0), (len(tab) - 1, 6), (WG, 4)):
        bad = tab.copy()
        bad[where] = 2**40
        with pytest.raises(p.VgaError) as e:
            ctx.variant_call_table(bad, letters)
        assert e.value.code == -4, where  # VGA_ERR_UNSUPPORTED


def test_many_random_rows_with_frequent_ties(ctx):
    tab, letters = random_table(100000, seed=8)
    want = variant_ref.call_table(tab, letters)
    ties = int((want["qual"] == 0).sum()) + int((want["ins_qual"] == 0).sum())
    print("calls", want["n_calls"], "of them with a tied genotype or insertion state", ties)
    assert want["n_calls"] > 10000 and ties > 100
    agree(ctx.variant_call_table(tab, letters), want, "1e5 rows")
    # other parameters move the ties elsewhere
    sub = slice(0, 20000)
    for error, min_depth, min_qual in ((512, 1, 0), (400, 7, 256), (8192, 12, 4096)):
        agree(ctx.variant_call_table(tab[sub], letters[sub], error, min_depth, min_qual),
              variant_ref.call_table(tab[sub], letters[sub], error, min_depth, min_qual), "E=%d" % error)


def test_lower_case_letters_and_n(ctx):
    tab, letters = random_table(3 * WG, seed=9, letters="ACGT")
    up = ctx.variant_call_table(tab, letters)
    low = ctx.variant_call_table(tab, letters.lower())
    assert variant_ref.same(up, low) is None and up["n_calls"] > 0
    agree(low, variant_ref.call_table(tab, letters.lower()), "lower case")
    got = ctx.variant_call_table(tab, "N" * len(tab))
    assert (got["n_tested"], got["n_calls"]) == (0, 0)
    mixed = "".join("n" if i % 3 == 0 else c for i, c in enumerate(letters))
    got = ctx.variant_call_table(tab, mixed)
    agree(got, variant_ref.call_table(tab, mixed), "every third base n")
    assert not (got["pos"] % 3 == 0).any()


def test_parameters_out_of_range(ctx):
    p = pkg()
    tab, letters = random_table(10, seed=10)
    for kw in ({"error": 256}, {"error": 8193}, {"error": 0}, {"min_depth": 0}):
        with pytest.raises(p.VgaError) as e:
            ctx.variant_call_table(tab, letters, **kw)
        assert e.value.code == -1, kw  # VGA_ERR_ARG
    agree(ctx.variant_call_table(tab, letters, error=257, min_depth=1, min_qual=0), variant_ref.call_table(tab, letters, 257, 1, 0), "the smallest values")
    L = p.binding.load_library()
    t = np.ascontiguousarray(tab)
    assert L.vga_variant_call_table(ctx.h, len(t), t.ctypes.data_as(C.POINTER(C.c_uint64)), letters.encode(), 1280, 4, 512, 5, None, None, None, None, None,
                                    None, None, None) == -1  # room for five calls and no array
    assert L.vga_variant_call_table(ctx.h, 5, None, None, 1280, 4, 512, 0, None, None, None, None, None, None, None, None) == -1  # rows and no table


# ---- 2. through a context, on DRB1 with a few hundred short reads
def short_reads(n, seed, reverse_fraction=0.0):
    return pkg().readsim.simulate_reads(DRB1, n, 400, 0.02, 0.01, 0.01, seed=seed, reverse_fraction=reverse_fraction)


def oracle_gaf(oracle, ix, seqs):
    return oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs)[1]


def count(c, seqs, map_params=None):
    b = c.batch(seqs)
    mo = b.map(map_params) if map_params is not None else b.map()
    al = b.align(mo)
    b.close()
    return al, mo


def check_context(c, a, gaf_texts, what):
    """variant_call() against the reference on pileup() of the same context and on the GAF texts counted so far"""
    counts, _, _ = c.pileup()
    got = c.variant_call()
    agree(got, variant_ref.call_table(counts, a["seq_fwd"]), what + ": against pileup()")
    agree(got, variant_ref.call_gaf("".join(gaf_texts), a["node_seq_idx"], a["seq_fwd"]), what + ": against the GAF")
    again, _, _ = c.pileup()
    assert np.array_equal(again, counts), "the call does not reset or change the counters"
    return got


def test_context_two_batches_and_a_reset(oracle, drb1):
    p = pkg()
    a = oracle_index_arrays(drb1)
    s1, s2 = [r.seq for r in short_reads(300, 61)], [r.seq for r in short_reads(200, 62)]
    g1, g2 = oracle_gaf(oracle, drb1, s1), oracle_gaf(oracle, drb1, s2)
    c = p.Context(0)
    try:
        upload_oracle_index(c, drb1)
        with pytest.raises(p.VgaError) as e:
            c.variant_call()
        assert e.value.code == -1  # VGA_ERR_ARG: no vga_pileup_begin
        c.pileup_begin()
        empty = c.variant_call()
        assert (empty["n_tested"], empty["n_calls"]) == (0, 0)
        count(c, s1)
        assert not any(t["name"].startswith("k_vc") for t in c.kernel_times()), "no call asked for: no kernel of it launched"
        first = check_context(c, a, [g1], "first batch")
        names = [t["name"] for t in c.kernel_times()]
        assert "k_vc_count" in names and "k_vc_scan" in names, names
        assert first["n_tested"] > 1000 and first["n_calls"] > 0
        # other parameters on the same counters
        agree(c.variant_call(error=600, min_depth=2, min_qual=256), variant_ref.call_gaf(g1, a["node_seq_idx"], a["seq_fwd"], 600, 2, 256), "other parameters")
        agree(c.variant_call(cap=1), first, "cap 1, asked again")
        count(c, s2)
        both = check_context(c, a, [g1, g2], "two batches")
        assert both["n_tested"] > first["n_tested"]
        c.pileup_reset()
        empty = c.variant_call()
        assert (empty["n_tested"], empty["n_calls"]) == (0, 0)
        count(c, s2)
        check_context(c, a, [g2], "after the reset")
        for kw in ({"error": 256}, {"error": 8193}, {"min_depth": 0}):
            with pytest.raises(p.VgaError) as e:
                c.variant_call(**kw)
            assert e.value.code == -1, kw
        c.pileup_end()
        with pytest.raises(p.VgaError) as e:
            c.variant_call()
        assert e.value.code == -1  # VGA_ERR_ARG: after vga_pileup_end
    finally:
        c.close()


@pytest.mark.parametrize("list_words", [None, "0"], ids=["lists on the device", "VGA_PILEUP_LIST_WORDS=0"])
def test_context_both_strands(oracle, ctx, drb1, monkeypatch, list_words):
    p = pkg()
    if list_words is not None:
        monkeypatch.setenv("VGA_PILEUP_LIST_WORDS", list_words)
    a = oracle_index_arrays(drb1)
    seqs = [r.seq for r in short_reads(300, 63, reverse_fraction=0.5)]
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    upload_oracle_index(ctx, drb1)
    ctx.pileup_begin()
    _, mo = count(ctx, seqs, map_params=mp)
    assert 0 < int(mo.strand.sum()) < len(seqs)
    chosen = [p.readsim.reverse_complement(s) if st else s for s, st in zip(seqs, mo.strand.tolist())]
    got = check_context(ctx, a, [oracle_gaf(oracle, drb1, chosen)], "both strands")
    assert got["n_calls"] > 0
    ctx.pileup_end()


# ---- 3. the executable
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
    a = oracle_index_arrays(drb1)
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain")])
    run(common + ["-o", os.path.join(d, "piled"), "--pileup"])
    assert not os.path.exists(os.path.join(d, "plain-variants.tsv")) and not os.path.exists(os.path.join(d, "piled-variants.tsv"))
    read = lambda name: open(os.path.join(d, name)).read()
    texts = {}
    for out, extra in (("one", []), ("two", ["--devices", "0,0", "--chunk-reads", "7"]), ("with", ["--pileup"]),
                       ("strict", ["--call-error", "2000", "--call-min-depth", "6", "--call-min-qual", "1024"])):
        pr = run(common + ["-o", os.path.join(d, out), "--call-variants"] + extra)
        # every other file is what it is without the switch
        assert read(out + "-chains.gaf") == read("plain-chains.gaf") and read(out + "-alignments.gaf") == read("plain-alignments.gaf"), out
        assert os.path.exists(os.path.join(d, out + "-pileup.tsv")) == (out == "with")
        kw = {"error": 2000, "min_depth": 6, "min_qual": 1024} if out == "strict" else {}
        want = variant_ref.call_gaf(read(out + "-alignments.gaf"), a["node_seq_idx"], a["seq_fwd"], **kw)
        texts[out] = read(out + "-variants.tsv")
        assert texts[out] == variant_ref.tsv(want, a["node_seq_idx"], a["seq_fwd"]), out
        assert "call-variants: %d bases tested, %d calls" % (want["n_tested"], want["n_calls"]) in pr.stderr, pr.stderr
        assert want["n_calls"] > 0, out
        assert sorted(os.listdir(d)).count(out + "-variants.tsv") == 1
    assert read("with-pileup.tsv") == read("piled-pileup.tsv")
    assert texts["two"] == texts["one"] == texts["with"] and texts["strict"] != texts["one"]
    assert {f[len("one"):] for f in os.listdir(d) if f.startswith("one-")} == {f[len("plain"):] for f in os.listdir(d) if f.startswith("plain-")} | {"-variants.tsv"}
