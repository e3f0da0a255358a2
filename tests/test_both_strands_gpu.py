"""vga_map_params.strands = VGA_STRANDS_BOTH (`vgaligner map --both-strands`) on the GPU.  The expected output of a read is
the forward-only output of the orientation the strand rule picks: the oracle's chain_anchors / map_reads on the read or on
its reverse complement.  The CLI check needs no oracle: the reverse complements of a read set, mapped with --both-strands,
give the forward records of the read set with '-' in column 5."""
import os

import numpy as np
import pytest

from helpers import DATA, ROOT, compare_map, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
MAP_FIELDS = ("anchor_off", "query_begin", "target_begin", "target_end", "curr_max", "chain_off", "chain_placeholder",
              "chain_anchor_off", "chain_anchor_idx")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


def both_params(emit_dp=1):
    p = pkg()
    mp = p.default_map_params()
    mp.emit_dp = emit_dp
    mp.strands = p.binding.VGA_STRANDS_BOTH
    return mp


def rc(s):
    return pkg().readsim.reverse_complement(s)


def rule(oracle, ix, s):
    """the strand rule of include/vga_hip.h on the oracle's chaining of s and of its reverse complement"""
    f, b = oracle.chain_anchors(ix, s), oracle.chain_anchors(ix, rc(s))
    f_real, b_real = not all(f.is_placeholder), not all(b.is_placeholder)
    return 1 if b_real and (not f_real or b.curr_max > f.curr_max) else 0


def check_map(oracle, ctx, ix, reads):
    """map parity of both mode; returns (batch, map result, the chosen sequences)"""
    seqs = [r.seq for r in reads]
    b = ctx.batch(seqs)
    mo = b.map(both_params(1))
    want = [rule(oracle, ix, s) for s in seqs]
    assert mo.strand is not None and mo.strand.tolist() == want
    chosen = [rc(s) if st else s for s, st in zip(seqs, want)]
    compare_map(oracle, ix, mo, chosen)
    # emit_dp = 0: the same coordinates and chains, nothing else
    m0 = b.map(both_params(0))
    assert m0.anchor_id is None and m0.max_chain_score is None and m0.best_pred_id is None
    for name in MAP_FIELDS + ("strand",):
        assert np.array_equal(getattr(m0, name), getattr(mo, name)), name
    # n_hits counts the records of both orientations; forward mode on the same batch is what it was
    fwd = b.map()
    assert fwd.strand is None
    assert mo.n_hits == fwd.n_hits + ctx.batch([rc(s) for s in seqs]).map().n_hits
    fresh = ctx.batch(seqs).map()
    for name in MAP_FIELDS + ("anchor_id", "max_chain_score", "best_pred_id"):
        assert np.array_equal(getattr(fwd, name), getattr(fresh, name)), name
    return b, mo, chosen


def recall(mo, reads, min_len=1500):
    idx = [i for i, r in enumerate(reads) if len(r.seq) >= min_len]
    hit = sum(1 for i in idx if int(mo.strand[i]) == (1 if reads[i].strand == "-" else 0))
    return hit / len(idx)


def check_align(oracle, ix, b, mo, names, chosen):
    al = b.align(mo)
    _, ag, st = oracle.map_reads(ix, names, chosen)
    lines = ag.splitlines()
    assert len(lines) == len(chosen)
    for r, ln in enumerate(lines):
        f = ln.split("\t")
        if f[5] == "*":
            assert not al.aligned[r], f"read {r} aligned on the GPU only"
            continue
        assert al.aligned[r], f"read {r} aligned on the CPU only"
        hs = al.path_handles[int(al.path_off[r]):int(al.path_off[r + 1])].tolist()
        assert "".join((">" if not (h & 1) else "<") + str(h >> 1) for h in hs) == f[5], f"read {r}: node path"
        assert f[12] == "as:i:-30 " + al.cs[r] + ",cg:Z:" + al.cigar[r], f"read {r}: cs / CIGAR"
        assert (int(f[6]), int(f[7]), int(f[8]), int(f[10])) == (
            int(al.path_length[r]), int(al.path_start[r]), int(al.path_end[r]), int(al.block_length[r]))
    assert al.poa_cells == st["poa_cells"] and al.poa_rows == st["poa_rows"]
    return al


def test_drb1_map_align_and_strand_recall(oracle, ctx, drb1, monkeypatch):
    """DRB1-3123: 300 x 1.5 kbp and 40 x 10 kbp reads, half of them reverse complements; map parity for all, alignment parity
    for a part of them on the device route and on the two host routes (the second on a batch whose reverse complement the
    alignment call has to build itself)"""
    sim = pkg().readsim.simulate_reads
    reads = (sim(DRB1, 300, 1500, 0.03, 0.03, 0.04, seed=31, reverse_fraction=0.5) +
             sim(DRB1, 40, 10000, 0.03, 0.03, 0.04, seed=32, reverse_fraction=0.5))
    assert 0.35 < sum(r.strand == "-" for r in reads) / len(reads) < 0.65
    upload_oracle_index(ctx, drb1)
    check = check_map(oracle, ctx, drb1, reads)
    assert recall(check[1], reads) >= 0.99
    part = reads[:100] + reads[300:308]
    names = [r.name for r in part]
    b = ctx.batch([r.seq for r in part])
    mp = b.map(both_params(0))
    pc = [rc(r.seq) if st else r.seq for r, st in zip(part, mp.strand.tolist())]
    assert int(mp.strand.sum()) > 20
    dev = check_align(oracle, drb1, b, mp, names, pc)
    for env in ("VGA_POA_TEXT", "VGA_SUBGRAPH"):
        monkeypatch.setenv(env, "host")
        bb = b if env == "VGA_POA_TEXT" else ctx.batch([r.seq for r in part])
        host = check_align(oracle, drb1, bb, mp, names, pc)
        monkeypatch.delenv(env)
        assert host.cigar == dev.cigar and host.path_handles.tolist() == dev.path_handles.tolist()


def test_config4_and_config5_map_parity(oracle, ctx, config4_gfa, config5_small_gfa):
    """the merged HLA graph (100 x 3 kbp) and the config-5 generator (100 x 2 kbp): map parity and strand recall; a sample of
    each through the alignment"""
    sim = pkg().readsim.simulate_reads
    for gfa, n, ln in ((config4_gfa, 100, 3000), (config5_small_gfa, 100, 2000)):
        ix = oracle.Index(oracle.Graph.from_gfa(gfa), 11)
        upload_oracle_index(ctx, ix)
        reads = sim(gfa, n, ln, 0.03, 0.03, 0.04, seed=33, reverse_fraction=0.5)
        _, mo, chosen = check_map(oracle, ctx, ix, reads)
        assert recall(mo, reads) >= 0.99
        k = 24
        bs = ctx.batch([r.seq for r in reads[:k]])
        check_align(oracle, ix, bs, bs.map(both_params(0)), [r.name for r in reads[:k]], chosen[:k])


def test_all_forward_reads_keep_forward_results(ctx, drb1):
    """config-3-style reads, all forward: both mode picks '+' for (nearly) all, and every '+' read's map and alignment fields
    equal forward mode's"""
    upload_oracle_index(ctx, drb1)
    reads = pkg().readsim.config3_reads(DRB1, 60)
    b = ctx.batch([r.seq for r in reads])
    fw, bo = b.map(), b.map(both_params(1))
    assert (bo.strand == 0).mean() >= 0.99
    plus = np.flatnonzero(bo.strand == 0).tolist()
    for r in plus:
        fa, fb = slice(int(fw.anchor_off[r]), int(fw.anchor_off[r + 1])), slice(int(bo.anchor_off[r]), int(bo.anchor_off[r + 1]))
        for name in ("anchor_id", "query_begin", "target_begin", "target_end", "max_chain_score", "best_pred_id"):
            assert np.array_equal(getattr(fw, name)[fa], getattr(bo, name)[fb]), (r, name)
        assert fw.curr_max[r] == bo.curr_max[r] and fw.chains_of(r) == bo.chains_of(r)
    af, ab = b.align(fw), b.align(bo)
    for r in plus:
        assert af.aligned[r] == ab.aligned[r] and af.cigar[r] == ab.cigar[r] and af.cs[r] == ab.cs[r]
        assert af.path_handles[int(af.path_off[r]):int(af.path_off[r + 1])].tolist() == \
            ab.path_handles[int(ab.path_off[r]):int(ab.path_off[r + 1])].tolist()
        assert (af.path_length[r], af.path_start[r], af.path_end[r], af.block_length[r], af.best_score[r]) == \
            (ab.path_length[r], ab.path_start[r], ab.path_end[r], ab.block_length[r], ab.best_score[r])


def test_refusals(ctx, drb1):
    p = pkg()
    upload_oracle_index(ctx, drb1)
    b = ctx.batch(["ACGT" * 50])
    mp = both_params()
    mp.only_forward = 0
    with pytest.raises(p.VgaError) as e:
        b.map(mp)
    assert e.value.code == -4
    mp = both_params()
    mp.strands = 7
    with pytest.raises(p.VgaError) as e:
        b.map(mp)
    assert e.value.code == -1


def _records(path):
    out = {}
    for ln in open(path).read().splitlines():
        f = ln.split("\t")
        out.setdefault(f[0], []).append(f)
    return out


def test_cli_reverse_complements_give_the_forward_records(tmp_path):
    """`vgaligner map --both-strands -D` on the reverse complements of S against `vgaligner map -D` on S: an alignment record
    differs in column 5 only, a chain record in column 5 and the flip of columns 3 / 4, placeholders not at all; two contexts
    and small chunks give the same files; a '-' read's validation record carries the sequence its CIGAR describes"""
    import subprocess

    p = pkg()
    d = str(tmp_path)
    reads = p.readsim.simulate_reads(DRB1, 400, 2000, 0.03, 0.03, 0.04, seed=55)
    fw, rv = os.path.join(d, "s.fa"), os.path.join(d, "rc.fa")
    with open(fw, "w") as f, open(rv, "w") as g:
        for r in reads:
            f.write(">%s\n%s\n" % (r.name, r.seq))
            g.write(">%s\n%s\n" % (r.name, rc(r.seq)))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    base = ["map", "-i", os.path.join(d, "drb1"), "-p", "abpoa", "-D", "-G", DRB1]
    run(base + ["-f", fw, "-o", os.path.join(d, "fw"), "-v", "-P", os.path.join(d, "fw.val")])
    one = run(base + ["-f", rv, "-o", os.path.join(d, "rv"), "--both-strands", "-v", "-P", os.path.join(d, "rv.val")])
    n_rev = int(one.stderr.split(" of 400 reads on the reverse strand")[0].split()[-1])
    assert n_rev >= 396
    a_fw, a_rv = _records(os.path.join(d, "fw-alignments.gaf")), _records(os.path.join(d, "rv-alignments.gaf"))
    c_fw, c_rv = _records(os.path.join(d, "fw-chains.gaf")), _records(os.path.join(d, "rv-chains.gaf"))
    minus = 0
    for r in reads:
        x, y = a_fw[r.name][0], a_rv[r.name][0]
        if y[4] == "-":
            minus += 1
            assert y[:4] + y[5:] == x[:4] + x[5:] and x[4] == "+", r.name
            L = int(x[1])
            assert len(c_fw[r.name]) == len(c_rv[r.name])
            for cx, cy in zip(c_fw[r.name], c_rv[r.name]):
                assert (cy[2], cy[3], cy[4]) == (str(L - int(cx[3])), str(L - int(cx[2])), "-") and cx[4] == "+"
                assert cy[:2] + cy[5:] == cx[:2] + cx[5:]
        elif all(c[5] == "*" for c in c_fw[r.name] + c_rv[r.name]):
            assert x == y and c_fw[r.name] == c_rv[r.name]
    assert minus == n_rev
    # validation records: a '-' record carries rc(rc(s)) = s, what the forward record of s carries
    vf = {b.split("\n")[0]: b for b in open(os.path.join(d, "fw.val")).read().split("\n\n") if b}
    vr = {b.split("\n")[0]: b for b in open(os.path.join(d, "rv.val")).read().split("\n\n") if b}
    for r in reads:
        if a_rv[r.name][0][4] == "-":
            assert vr[r.name] == vf[r.name], r.name
    two = run(base + ["-f", rv, "-o", os.path.join(d, "rv2"), "--both-strands", "--devices", "0,0", "--chunk-reads", "64"])
    assert "2 GPU context(s)" in two.stderr and ("%d of 400 reads on the reverse strand" % n_rev) in two.stderr
    for suffix in ("-chains.gaf", "-alignments.gaf"):
        assert open(os.path.join(d, "rv" + suffix)).read() == open(os.path.join(d, "rv2" + suffix)).read()
