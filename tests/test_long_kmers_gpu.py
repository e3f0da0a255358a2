"""k-mers of 16 to 32 bases on the GPU: the hashed probe table (rs-vgaligner_amd/csrc/vga_probe_hash.hpp), its insert kernel
and K1's 64-bit-key variant, through vga_index_upload / vga_map_batch / vga_align_batch and the `vgaligner` executable,
against the CPU oracle bit for bit.  Without the hashed table every test that uploads an index of k >= 16 stops there (VgaError -4)."""
import os
import random
import subprocess

import numpy as np
import pytest

from helpers import DATA, ROOT, compare_map, pkg, upload_oracle_index
from test_both_strands_gpu import both_params, rc, rule
from test_gpu_parity import _check_align

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
TEST_GFA = os.path.join(DATA, "test.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
MAP_FIELDS = ("anchor_off", "anchor_id", "query_begin", "target_begin", "target_end", "max_chain_score", "best_pred_id", "curr_max",
              "chain_off", "chain_placeholder", "chain_anchor_off", "chain_anchor_idx")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1_graph(oracle):
    return oracle.Graph.from_gfa(DRB1)


def _params(only_forward=1):
    mp = pkg().default_map_params()
    mp.emit_dp = 1
    mp.only_forward = only_forward
    return mp


def _no_placeholder(oracle, ix, seqs):
    """the condition on the inputs: under the oracle every read has a real chain, so no parity check compares empty chains"""
    n_anchors = 0
    for r, s in enumerate(seqs):
        ref = oracle.chain_anchors(ix, s)
        assert ref.chains and not any(ref.is_placeholder), f"read {r} is a placeholder under the oracle"
        n_anchors += len(ref.sorted_anchors)
    return n_anchors


def _map_parity(oracle, ctx, ix, seqs):
    want = _no_placeholder(oracle, ix, seqs)
    upload_oracle_index(ctx, ix)
    mo = ctx.batch(seqs).map(_params())
    print(f"k {ix.k}: {mo.n_anchors} anchors on the GPU, {want} in the oracle, {len(seqs)} reads")
    assert mo.n_anchors == want
    compare_map(oracle, ix, mo, seqs)
    return mo


# ---- 1. map parity
@pytest.mark.parametrize("k", [16, 19, 24, 31, 32])
def test_map_parity_drb1(oracle, ctx, drb1_graph, k):
    seqs = [r.seq for r in pkg().readsim.config3_reads(DRB1, 64, 3000)]
    _map_parity(oracle, ctx, oracle.Index(drb1_graph, k), seqs)


@pytest.mark.parametrize("k", [16, 31])
def test_map_parity_test_gfa(oracle, ctx, k):
    seqs = [r.seq for r in pkg().readsim.simulate_reads(TEST_GFA, 8, 60, 0, 0, 0, seed=3)]
    _map_parity(oracle, ctx, oracle.Index(oracle.Graph.from_gfa(TEST_GFA), k), seqs)


def test_map_parity_synthetic_pangenome_k19(oracle, ctx, tmp_path):
    """5 354 short nodes: most 19-mers span several of them"""
    gfa = str(tmp_path / "syn100k.gfa")
    pkg().readsim.synth_pangenome(gfa, total_bp=100000)
    seqs = [r.seq for r in pkg().readsim.config3_reads(gfa, 32, 3000)]
    _map_parity(oracle, ctx, oracle.Index(oracle.Graph.from_gfa(gfa), 19), seqs)


# ---- 2. every orientation, both strands
@pytest.mark.parametrize("k", [16, 32])
def test_all_orientations(oracle, ctx, drb1_graph, k):
    ix = oracle.Index(drb1_graph, k)
    upload_oracle_index(ctx, ix)
    seqs = [r.seq for r in pkg().readsim.config3_reads(DRB1, 32, 3000)]
    seqs += [rc(s) for s in seqs[:8]]  # (reverse complements: their anchors are the records of the reverse strand)
    mo = ctx.batch(seqs).map(_params(only_forward=0))
    assert mo.n_anchors > 0 and int(((mo.target_begin | mo.target_end) >> 31).sum()) > 0  # (reverse-strand records are there)
    compare_map(oracle, ix, mo, seqs, only_forward=False)


def test_both_strands_k19(oracle, ctx, drb1_graph):
    """the chosen orientation's result equals the oracle's on that sequence (as tests/test_both_strands_gpu.py checks it)"""
    ix = oracle.Index(drb1_graph, 19)
    upload_oracle_index(ctx, ix)
    reads = pkg().readsim.simulate_reads(DRB1, 64, 3000, 0.03, 0.03, 0.04, seed=31, reverse_fraction=0.5)
    assert 0.25 < sum(r.strand == "-" for r in reads) / len(reads) < 0.75
    seqs = [r.seq for r in reads]
    mo = ctx.batch(seqs).map(both_params(1))
    want = [rule(oracle, ix, s) for s in seqs]
    assert mo.strand is not None and mo.strand.tolist() == want
    assert 0 < sum(want) < len(want)
    assert want == [1 if r.strand == "-" else 0 for r in reads]
    compare_map(oracle, ix, mo, [rc(s) if st else s for s, st in zip(seqs, want)])


# ---- 3. align parity
@pytest.mark.parametrize("k", [19, 32])
def test_align_parity(oracle, ctx, drb1_graph, k):
    ix = oracle.Index(drb1_graph, k)
    upload_oracle_index(ctx, ix)
    reads = pkg().readsim.config3_reads(DRB1, 16, 3000)
    al = _check_align(oracle, ctx, ix, reads)
    assert int(np.asarray(al.aligned).sum()) == len(reads)
    # the GAF text of the host library on its own index of the same k
    names, seqs = [r.name for r in reads], [r.seq for r in reads]
    hi = pkg().HostIndex.build_from_gfa(DRB1, k)
    hi.upload(ctx)
    cg, ag, n_al = hi.map_reads(ctx, names, seqs, also_align=True)
    ocg, oag, _ = oracle.map_reads(ix, names, seqs)
    assert cg == ocg, "chains GAF"
    assert ag == oag, "alignments GAF"
    assert n_al == len(reads)


# ---- 4. the edges of the key space
def _write_gfa(path, nodes):
    """a chain of forward nodes with one path over all of them"""
    lines = ["H\tVN:Z:1.0"] + [f"S\t{i + 1}\t{s}" for i, s in enumerate(nodes)]
    lines += [f"L\t{i + 1}\t+\t{i + 2}\t+\t0M" for i in range(len(nodes) - 1)]
    lines.append("P\tp\t" + ",".join(f"{i + 1}+" for i in range(len(nodes))) + "\t*")
    open(path, "w").write("\n".join(lines) + "\n")
    return path


def _mixed(rng, n):
    """random bases without a run of more than 3 equal ones (no chance poly-A / poly-T k-mer)"""
    out = []
    while len(out) < n:
        c = rng.choice("ACGT")
        if out[-3:] != [c] * 3:
            out.append(c)
    return "".join(out)


@pytest.mark.parametrize("k", [16, 32])
def test_edges_of_the_key_space(oracle, ctx, tmp_path, k):
    rng = random.Random(1632)
    nodes = [_mixed(rng, 70), "A" * 40, _mixed(rng, 70), "T" * 40, _mixed(rng, 70)]
    whole = "".join(nodes)
    ix = oracle.Index(oracle.Graph.from_gfa(_write_gfa(str(tmp_path / "edges.gfa"), nodes)), k)
    upload_oracle_index(ctx, ix)
    with_n = "".join("N" if i % 20 == 19 else c for i, c in enumerate(whole))
    seqs = [whole, whole[50:130], whole[160:240], with_n, "A" * 40, "T" * 40,
            whole[5:5 + k - 1], whole[5:5 + k], whole[5:5 + k + 1], whole[60:60 + k + 2], "N" * 50]
    mo = ctx.batch(seqs).map(_params())
    compare_map(oracle, ix, mo, seqs)
    # key 0 (all A) and the key with every bit set (all T) are found, with the oracle's positions
    for base, read in (("A", 0), ("T", 0), ("A", 1), ("T", 2), ("A", 4), ("T", 5)):
        want = [x for x in oracle.chain_anchors(ix, seqs[read]).sorted_anchors
                if seqs[read][x.query_begin:x.query_begin + k] == base * k]
        a0, a1 = int(mo.anchor_off[read]), int(mo.anchor_off[read + 1])
        got = [i for i in range(a0, a1) if seqs[read][int(mo.query_begin[i]):int(mo.query_begin[i]) + k] == base * k]
        assert len(want) >= 40 - k + 1 and len(got) == len(want), (base, read, len(got), len(want))
        assert sorted((int(mo.query_begin[i]), int(mo.target_begin[i]), int(mo.target_end[i])) for i in got) == \
            sorted((x.query_begin, x.target_begin[1], x.target_end[1]) for x in want)
    a = mo.anchor_off
    if k == 32:  # (N every 20 bases: no clean 32-mer)
        assert int(a[4]) - int(a[3]) == 0
    else:
        assert int(a[4]) - int(a[3]) > 0
    assert int(a[7]) - int(a[6]) == 0 and int(a[8]) - int(a[7]) == 1 and int(a[9]) - int(a[8]) == 2 and int(a[10]) - int(a[9]) == 3
    assert int(a[11]) - int(a[10]) == 0
    # every orientation on the same table
    mo_all = ctx.batch(seqs).map(_params(only_forward=0))
    compare_map(oracle, ix, mo_all, seqs, only_forward=False)

    # a graph without poly-A / poly-T: key 0 and ~0 are absent, and an empty slot (all bits set) matches neither
    plain = [_mixed(rng, 90), _mixed(rng, 90)]
    ix2 = oracle.Index(oracle.Graph.from_gfa(_write_gfa(str(tmp_path / "plain.gfa"), plain)), k)
    upload_oracle_index(ctx, ix2)
    seqs2 = ["A" * 100, "T" * 100, "".join(plain), "A" * k, "T" * k]
    for only_forward in (1, 0):
        m2 = ctx.batch(seqs2).map(_params(only_forward))
        compare_map(oracle, ix2, m2, seqs2, only_forward=bool(only_forward))
        assert int(m2.anchor_off[2]) == 0 and int(m2.anchor_off[3]) > 0 and int(m2.anchor_off[5]) == int(m2.anchor_off[3])


def test_short_reads_chains_gaf_k32(oracle, tmp_path):
    """reads barely longer than k through the executable: the chains GAF's query end (query_begin + k) against the oracle's
    text, and the frame arithmetic of --both-strands (the reverse complements give the forward records, flipped)"""
    pkg()
    k, d = 32, str(tmp_path)
    rng = random.Random(32)
    nodes = [_mixed(rng, 60), _mixed(rng, 45), _mixed(rng, 80)]
    whole = "".join(nodes)
    gfa = _write_gfa(os.path.join(d, "short.gfa"), nodes)
    reads = [("r%d" % n, whole[off:off + k + extra]) for n, (off, extra) in enumerate([(3, 2), (40, 3), (51, 5), (90, 8), (100, 40), (7, 0), (9, 1)])]
    fw, rv = os.path.join(d, "s.fa"), os.path.join(d, "rc.fa")
    with open(fw, "w") as f, open(rv, "w") as g:
        for name, s in reads:
            f.write(">%s\n%s\n" % (name, s))
            g.write(">%s\n%s\n" % (name, rc(s)))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr

    run(["index", "-i", gfa, "-k", str(k), "-o", os.path.join(d, "short")])
    base = ["map", "-i", os.path.join(d, "short"), "-p", "abpoa", "-D", "-G", gfa]
    run(base + ["-f", fw, "-o", os.path.join(d, "fw")])
    run(base + ["-f", rv, "-o", os.path.join(d, "rv"), "--both-strands"])
    ix = oracle.Index(oracle.Graph.from_gfa(gfa), k)
    ocg, oag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    cg = open(os.path.join(d, "fw-chains.gaf")).read()
    assert cg == ocg and open(os.path.join(d, "fw-alignments.gaf")).read() == oag
    real = [ln.split("\t") for ln in cg.splitlines() if ln.split("\t")[5] != "*"]
    assert len(real) == 5 and all(int(f[3]) <= int(f[1]) for f in real)
    assert any(int(f[3]) == int(f[1]) == k + 2 for f in real)  # (3 anchors: the last k-mer ends with the read)
    rcg = [ln.split("\t") for ln in open(os.path.join(d, "rv-chains.gaf")).read().splitlines()]
    fcg = [ln.split("\t") for ln in cg.splitlines()]
    assert len(rcg) == len(fcg)
    for x, y in zip(fcg, rcg):
        if x[5] == "*":
            assert x == y
            continue
        L = int(x[1])
        assert (y[2], y[3], y[4]) == (str(L - int(x[3])), str(L - int(x[2])), "-") and x[4] == "+"
        assert y[:2] + y[5:] == x[:2] + x[5:]
    for x, y in zip(oag.splitlines(), open(os.path.join(d, "rv-alignments.gaf")).read().splitlines()):
        x, y = x.split("\t"), y.split("\t")
        assert y[:4] + y[5:] == x[:4] + x[5:] and (x[5] == "*" or (x[4], y[4]) == ("+", "-"))


# ---- 5. collisions: the two kinds of table on one index
def test_k32_drb1_table_is_large(oracle, drb1_graph):
    """about 1.48 million distinct 32-mers: probe sequences of every length occur in test_map_parity_drb1[32]"""
    assert oracle.Index(drb1_graph, 32).n_kmers > 1_400_000


@pytest.mark.parametrize("k", [11, 15])
def test_hashed_table_equals_direct_table(oracle, drb1_graph, monkeypatch, k):
    p = pkg()
    ix = oracle.Index(drb1_graph, k)
    reads = p.readsim.simulate_reads(DRB1, 256, 1500, 0.03, 0.03, 0.04, seed=1115, reverse_fraction=0.5)
    seqs = [r.seq for r in reads]
    modes = [("forward", _params())] + ([("all orientations", _params(only_forward=0))] if k <= 13 else []) + [("both strands", both_params(1))]
    direct, hashed = p.Context(0), p.Context(0)
    try:
        monkeypatch.delenv("VGA_PROBE_TABLE", raising=False)
        upload_oracle_index(direct, ix)
        monkeypatch.setenv("VGA_PROBE_TABLE", "hash")  # read at upload time
        upload_oracle_index(hashed, ix)
        monkeypatch.delenv("VGA_PROBE_TABLE")
        bd, bh = direct.batch(seqs), hashed.batch(seqs)
        for what, mp in modes:
            md, mh = bd.map(mp), bh.map(mp)
            assert md.n_anchors == mh.n_anchors and md.n_anchors > 0, what
            for name in MAP_FIELDS + (("strand",) if mp.strands else ()):
                assert np.array_equal(getattr(md, name), getattr(mh, name)), (what, name)
        if k > 13:  # the refusal of only_forward = 0 at k = 14 and 15 stays, whichever table is loaded
            for b in (bd, bh):
                with pytest.raises(p.VgaError) as e:
                    b.map(_params(only_forward=0))
                assert e.value.code == -4 and "k <= 13" in str(e.value)
        compare_map(oracle, ix, bh.map(_params()), seqs)
    finally:
        direct.close()
        hashed.close()


# ---- 6. the executable
def test_cli_k19(oracle, drb1_graph, tmp_path):
    p = pkg()
    d = str(tmp_path)
    reads = p.readsim.config3_reads(DRB1, 32, 3000)
    fa = os.path.join(d, "r.fa")
    with open(fa, "w") as f:
        for r in reads:
            f.write(">%s\n%s\n" % (r.name, r.seq))

    def run(args, ok=True):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert (pr.returncode == 0) == ok, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "19", "-o", os.path.join(d, "drb1")])
    ocg, oag, _ = oracle.map_reads(oracle.Index(drb1_graph, 19), [r.name for r in reads], [r.seq for r in reads])
    assert sum(1 for ln in oag.splitlines() if ln.split("\t")[5] != "*") == len(reads)
    base = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    for out, extra in (("one", []), ("two", ["--devices", "0,0", "--chunk-reads", "10"])):
        run(base + ["-o", os.path.join(d, out)] + extra)
        assert open(os.path.join(d, out + "-chains.gaf")).read() == ocg, out
        assert open(os.path.join(d, out + "-alignments.gaf")).read() == oag, out
    # the k-mer half of the index on the GPU stays at k <= 15 and says where longer k-mers are built
    pr = run(["index", "--device", "0", "-i", DRB1, "-k", "19", "-o", os.path.join(d, "dev19")], ok=False)
    assert "host builder" in pr.stderr
    assert not os.path.exists(os.path.join(d, "dev19.idx")) and not os.path.exists(os.path.join(d, "dev19"))


# ---- 7. refusals, and an index after another
def test_k33_is_refused_and_the_next_index_replaces_the_tables(oracle, drb1_graph):
    p = pkg()
    c = p.Context(0)
    try:
        seqs = [r.seq for r in p.readsim.config3_reads(DRB1, 8, 3000)]
        upload_oracle_index(c, oracle.Index(drb1_graph, 19))  # a loaded context first: the refusal must unload it
        with pytest.raises(p.VgaError) as e:
            upload_oracle_index(c, oracle.Index(drb1_graph, 33))
        assert e.value.code == -4 and "1..32" in str(e.value)
        with pytest.raises(p.VgaError) as e:
            c.batch(seqs).map()
        assert e.value.code == -5
        ix19, ix11 = oracle.Index(drb1_graph, 19), oracle.Index(drb1_graph, 11)
        upload_oracle_index(c, ix19)
        compare_map(oracle, ix19, c.batch(seqs).map(_params()), seqs)
        upload_oracle_index(c, ix11)
        compare_map(oracle, ix11, c.batch(seqs).map(_params()), seqs)
        compare_map(oracle, ix11, c.batch(seqs).map(_params(only_forward=0)), seqs, only_forward=False)
        upload_oracle_index(c, ix19)
        compare_map(oracle, ix19, c.batch(seqs).map(_params()), seqs)
    finally:
        c.close()
