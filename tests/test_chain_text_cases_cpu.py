"""tests/chain_text_cases.py without a GPU: the reference's own text shows that the cases hold every condition they are there for
(a case that lost its condition would leave tests/test_chain_text_gpu.py green and blind), and the reference itself equals column
6 of the oracle's chains GAF on real reads."""
import os

import numpy as np
import pytest

import chain_text_cases as ctc
from helpers import DATA, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
TEST_GFA = os.path.join(DATA, "test.gfa")


@pytest.fixture(scope="module")
def texts():
    """{case name: [text per chain]}, computed once"""
    return {c.name: ctc.reference(c) for c in ctc.all_cases()}


def fields(text):
    """[(fn, fo, ln, lo) as the decimal strings of the text]; the anchors must tile the text"""
    found = ctc.ANCHOR_RE.findall(text)
    assert b"".join(b"(>%s:%s,>%s:%s)," % f for f in found) == text
    return found


def anchor_lengths(text):
    return [len(b"(>%s:%s,>%s:%s)," % f) for f in fields(text)]


def test_every_digit_count_and_both_sides_of_every_decimal_edge(texts):
    seen = [set(), set(), set(), set()]
    for chain in texts["decimal-edges"]:
        for f in fields(chain):
            for k in range(4):
                seen[k].add(int(f[k]))
    for k, (name, edges, most) in enumerate((("first node", ctc.ID_EDGES, 7), ("first offset", ctc.OFFSET_EDGES, 9),
                                             ("last node", ctc.ID_EDGES, 7), ("last offset", ctc.OFFSET_EDGES, 9))):
        assert {len(str(v)) for v in seen[k]} == set(range(1, most + 1)), name
        for e in edges:
            assert e - 1 in seen[k] and e in seen[k], (name, e)
    assert ctc.OFFSET_EDGES[-1] == 10 ** 8 and ctc.ID_EDGES[-1] == 10 ** 6


def test_edge_positions():
    c, g = ctc.case("decimal-edges"), ctc.digits_graph()
    assert (g.n_nodes, g.seq_length) == (ctc.LAST_NODE, 100000001 + sum(ctc.SMALL_NODES) + ctc.LAST_NODE - 9)
    assert [g.node_length(i) for i in range(1, 11)] == [100000001, 1, 2, 10, 11, 100, 1001, 10001, 1, 1]
    tb, te = c.target_begin.astype(np.int64), c.target_end.astype(np.int64)
    fn, fo, ln, lo = ctc.anchor_numbers(g.node_start, tb, te)
    last_base = lo == np.array([g.node_length(int(n)) for n in ln]) - 1
    first_last = fo == np.array([g.node_length(int(n)) for n in fn]) - 1
    assert (tb == 0).any() and (te == g.seq_length).any()
    assert (first_last & (ln == fn + 1) & (lo == 0)).any(), "the last base of a node to the first base of the next"
    assert (last_base & (np.array([g.node_length(int(n)) for n in ln]) > 1)).any(), "an inclusive end on the last base of a node"
    assert (te - tb == 1).any(), "a one-base anchor"
    assert ((fn == 1) & (ln == g.n_nodes)).any(), "node 1 to the last node"
    assert (ln - fn > 1000).any(), "an anchor over many nodes"


def test_text_lengths_and_rounds(texts):
    chains = texts["text-lengths"]
    assert {n for ch in chains for n in anchor_lengths(ch)} == set(range(ctc.SHORTEST, ctc.LONGEST + 1))
    assert (ctc.SHORTEST, ctc.LONGEST) == (len(b"(>1:0,>1:0),"), len(b"(>1:100000000,>1:100000000),"))
    rounds = [anchor_lengths(ch)[at:at + 64] for ch in chains for at in range(0, len(anchor_lengths(ch)), 64)]
    assert any(len(r) == 64 and len(set(r)) >= 3 for r in rounds), "a round of 64 with at least three text lengths"
    assert any(len(set(r)) >= 10 and len({sum(r[:i]) % 4 for i in range(64)}) == 4 for r in rounds if len(r) == 64)
    by_chain = [anchor_lengths(ch) for ch in chains]
    assert any(a[:64] == [ctc.LONGEST] * 64 and a[64:] == [ctc.SHORTEST] * 64 for a in by_chain), "all long, then all short"
    assert any(a[:64] == [ctc.SHORTEST] * 64 and a[64:] == [ctc.LONGEST] * 64 for a in by_chain)


def test_chain_shapes(texts):
    c = ctc.case("chain-shapes")
    counts = [len(fields(t)) for t in texts["chain-shapes"]]
    assert sorted(n for n in counts if n) == sorted(ctc.MEMBER_COUNTS + (2,))
    ph = c.chain_placeholder.tolist()
    assert ph[0] == 1 and ph[-1] == 1 and 1 in ph[1:-1] and [n for n, p in zip(counts, ph) if p] == [0] * sum(ph)
    per_read = np.diff(c.chain_off.astype(np.int64))
    assert c.n_reads >= 4 and per_read.max() >= 3 and (c.anchor_off[:-1] > 0).sum() >= 3
    assert (np.diff(c.anchor_off.astype(np.int64)) == 0).any(), "a read with no anchors"
    mid = [r for r in range(c.n_reads) if per_read[r] >= 3 and 1 in ph[int(c.chain_off[r]) + 1:int(c.chain_off[r + 1]) - 1]]
    assert mid, "a placeholder between two chains of one read"
    for ch in range(c.n_chains):
        if ph[ch]:
            continue
        idx = c.chain_anchor_idx[int(c.chain_anchor_off[ch]):int(c.chain_anchor_off[ch + 1])].astype(np.int64)
        assert (np.diff(idx) > 0).all()
        if len(idx) >= 63:
            assert idx[0] > 0 and (np.diff(idx) > 1).any(), "members skip anchors and do not start at the read's first"


def test_chain_counts(texts):
    for n in ctc.CHAIN_COUNTS:
        t = texts["chains-%d" % n]
        assert len(t) == n and all(1 <= len(fields(x)) <= 3 for x in t)
    assert ctc.CHAIN_COUNTS == (1, 8191, 8192, 8193, 40000) and 8192 == 32 * 256
    big = ctc.case("chains-40000")
    assert len({len(fields(x)) for x in texts["chains-40000"]}) == 3 and np.diff(big.chain_off.astype(np.int64)).max() > 1
    assert texts["no-chains"] == [] and ctc.case("no-chains").n_reads == 2
    only = ctc.case("only-placeholders")
    assert only.n_chains == 3 and only.n_anchors > 0 and only.chain_placeholder.all() and texts["only-placeholders"] == [b""] * 3
    assert len(only.chain_anchor_idx) == 0


def test_the_result_object_points_at_the_case():
    c = ctc.case("chain-shapes")
    m = c.result()
    assert (m.n_reads, m.n_anchors, m.n_chains) == (c.n_reads, c.n_anchors, c.n_chains) and m._ptr.contents.n_chains == c.n_chains
    assert [m.target_begin[i] for i in range(c.n_anchors)] == c.target_begin.tolist()
    assert [m.chain_anchor_off[i] for i in range(c.n_chains + 1)] == c.chain_anchor_off.tolist()
    assert not m.anchor_id and not m.query_begin and not m.strand


def test_the_message_names_chain_anchor_and_numbers(texts):
    c = ctc.case("text-lengths")
    want = texts["text-lengths"]
    assert ctc.describe_first_difference(c, list(want), want) is None
    at = next(i for i, t in enumerate(want) if len(fields(t)) == 200)
    parts = fields(want[at])
    cut = sum(anchor_lengths(want[at])[:70])
    bad = list(want)
    bad[at] = want[at][:cut + 3] + b"9" + want[at][cut + 4:]
    msg = ctc.describe_first_difference(c, bad, want)
    f = parts[70]
    assert "chain %d " % at in msg and "its anchor 70 " in msg
    assert "first node %d offset %d, last node %d offset %d" % tuple(int(x) for x in f) in msg


# ---------------------------------------------------------------- the reference against the oracle
def oracle_case(oracle, ix, seqs):
    """path_column over the oracle's own chains against column 6 of its chains GAF, line by line"""
    node_start = [x[0] for x in ix.node_ref()]
    mp = oracle.default_map_params(also_align=False)
    lines = oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, mp)[0].splitlines()
    at = two = placeholders = 0
    for s in seqs:
        res = oracle.chain_anchors(ix, s)
        sa = res.sorted_anchors
        tb, te = [a.target_begin[1] for a in sa], [a.target_end[1] for a in sa]
        pos_of_id = {a.id: i for i, a in enumerate(sa)}
        two += len(res.chains) >= 2
        for ph, ch in zip(res.is_placeholder, res.chains):
            col = lines[at].split("\t")[5]
            at += 1
            if ph:
                placeholders += 1
                assert col == "*" and not ch
                continue
            assert ctc.path_column(node_start, tb, te, [pos_of_id[a.id] for a in ch]) == col.encode()
    assert at == len(lines)
    return two, placeholders


def test_reference_equals_the_oracles_chains_gaf_on_drb1(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    src = pkg().readsim.simulate_reads(DRB1, 6, 700, 0.02, 0.02, 0.02, seed=23)
    seqs = [r.seq for r in src] + [r.seq[:500] + r.seq[:500] for r in src] + ["ACGTTGCA", src[0].seq[:300] * 3]
    two, placeholders = oracle_case(oracle, ix, seqs)
    assert two >= 3 and placeholders >= 1


def test_reference_equals_the_oracles_chains_gaf_on_test_gfa(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(TEST_GFA), 11)
    seqs = [s for _, s in oracle.read_seqs_from_file(os.path.join(DATA, "test.fq"))]
    seqs += [s for _, s in oracle.read_seqs_from_file(os.path.join(DATA, "multiple-read-test.fa"))]
    assert seqs
    oracle_case(oracle, ix, seqs + ["ACGT"])
