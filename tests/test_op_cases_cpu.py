"""tests/op_cases.py produces what it is there for -- judged from the oracle's alignments GAF alone, so that
tests/test_op_cases_gpu.py cannot pass vacuously: every event kind on every lane of a 64-operation block, the closing operation
alone in a block, second and last in one, runs that hold whole blocks or end on a block edge, run lengths on both sides of every
digit count up to five, every kind of first and last operation, N in every role, a block that is mostly node entries."""
import collections

import numpy as np
import pytest

import coverage_ref
import op_cases as M
import pileup_ref
from helpers import oracle_index_arrays

LANES = set(range(64))


@pytest.fixture(scope="module")
def sets(oracle, tmp_path_factory):
    """name -> the oracle's side of a case set, computed once"""
    return M.oracle_side(oracle, tmp_path_factory.mktemp("op_cases"))


def records(sets, *names):
    return [r for n in (names or sets) for r in sets[n].records]


def all_runs(recs):
    """(record, kind, first f, length) of every run of equal column kinds"""
    return [(r, k, f, n) for r in recs for k, f, n in M.runs(r)]


def holds_block(f, n, blocks=1):
    """the columns f .. f + n - 1 hold `blocks` whole blocks of 64"""
    return -(-f // 64) * 64 + 64 * blocks <= f + n


def m_runs(rec):
    """the CIGAR M runs of a record as (first f, length), from the columns"""
    out, f = [], 0
    for n, c in rec.cigar:
        if c == "M":
            out.append((f, n))
        f += n
    return out


def test_sets_are_well_formed(sets):
    assert list(sets) == ["drb5-digits", "drb5-edges", "drb1-runs", "drb1-sweep", "drb1-entries", "synth-nodes", "drb1-both-strands"]
    assert set(M.BLOCK_EDGE_SETS) <= set(sets)
    for name, s in sets.items():
        assert 1 <= len(s.case.reads) <= 128 and s.case.k == 11
        long_reads = [r for r in s.case.reads if len(r) > 2500]
        assert all(set(r) <= set("ACGTN") for r in s.case.reads)
        assert not long_reads or (s.case.graph == "drb5" and len(long_reads) <= 3), name
    assert sum(len(s.case.reads) for s in sets.values()) <= 260


def test_every_read_is_aligned(sets):
    for name, s in sets.items():
        assert len(s.records) == len(s.case.reads), name
        assert all(r is not None for r in s.records), (name, [i for i, r in enumerate(s.records) if r is None])
        for r, read in zip(s.records, M.forward_reads(s.case)):
            assert sum(k != "D" for k, _, _ in r.cols) == len(read), (name, r.name)


def test_lane_sweep(sets):
    """every event kind on every lane.  The operation that ends a run is the first one behind it -- the lane that writes the
    run's text in k_poa_text; behind the last run that is the closing operation."""
    lanes = collections.defaultdict(set)
    for r, k, f, n in all_runs(records(sets)):
        if k == "X":
            lanes["mismatch"] |= {(f + j) % 64 for j in range(n)}
        if k in "ID":
            lanes["first of a run of " + k].add(f % 64)
        if k in "EID":
            lanes["end of a run of " + k].add((f + n) % 64)
    for r in records(sets):
        lanes["node entry"] |= {f % 64 for f, _, _ in r.entries}
    assert len(lanes) == 7
    for kind, seen in lanes.items():
        assert seen == LANES, (kind, sorted(LANES - seen))
    # the sweep set alone does it for the insertion directly behind a deletion
    behind = {f % 64 for r in records(sets, "drb1-sweep") for (k0, _, _), (k1, f, _) in zip(M.runs(r), M.runs(r)[1:]) if (k0, k1) == ("D", "I")}
    assert behind == LANES, sorted(LANES - behind)


def test_closing_operation(sets):
    nops = {len(r.cols) % 64 for r in records(sets, "drb5-edges", "drb5-digits")}
    assert {0, 1, 63} <= nops, nops
    # (and on DRB1, where the pileup lists of a call fit the buffer that k_pu_events writes to: see test_op_cases_gpu.py)
    assert {0, 1, 63} <= {len(r.cols) % 64 for r in records(sets, "drb1-sweep")}
    assert 12856 % 64 == 56 and all(len(r.cols) == 12856 + sum(k == "I" for k, _, _ in r.cols) for r in records(sets, "drb5-edges", "drb5-digits"))


def test_runs_against_blocks(sets):
    rr = all_runs(records(sets, *M.BLOCK_EDGE_SETS))
    assert any(k == "E" and holds_block(f, n, 2) for _, k, f, n in rr), "an = run over two whole blocks"
    # closed by a mismatch, an insertion, a deletion at lane 0, the run coming from the block before (c_erun)
    for closer in "XID":
        assert any(k == "E" and n >= 64 and (f + n) % 64 == 0 and f + n < len(r.cols) and r.cols[f + n][0] == closer for r, k, f, n in rr), closer
    assert any(k == "E" and n >= 64 and f + n == len(r.cols) and (f + n) % 64 == 0 for r, k, f, n in rr), "... and by the closing operation"
    for kind in "ID":
        assert any(k == kind and holds_block(f, n) for _, k, f, n in rr), kind + " run that holds a whole block"
        assert any(k == kind and f % 64 == 0 and n >= 64 for _, k, f, n in rr), kind + " run that is a whole block from lane 0 on"
        assert any(k == kind and f % 64 == 63 and n >= 2 for _, k, f, n in rr), kind + " run whose second operation is at lane 0"
    behind = collections.defaultdict(set)
    for r in records(sets):
        for (k0, _, _), (k1, f, _) in zip(M.runs(r), M.runs(r)[1:]):
            if k1 == "I" and f % 64 == 0:
                behind[k0].add(r.name)
    assert behind["E"] and behind["D"], "an insertion run at lane 0 directly behind a match / behind a deletion"
    at63 = at0 = pair = False
    for r in records(sets, *M.BLOCK_EDGE_SETS):
        for f, n in m_runs(r):
            xs = {g for g in range(f, f + n) if r.cols[g][0] == "X"}
            at63 |= any(g % 64 == 63 and g + 1 < f + n for g in xs)
            at0 |= any(g % 64 == 0 and g > f for g in xs)
            pair |= any(g % 64 == 63 and g + 1 in xs for g in xs)
    assert at63 and at0 and pair, "an M run that crosses a block edge with a mismatch at lane 63 / at lane 0 / at both"


def test_digits(sets):
    recs = records(sets, *M.BLOCK_EDGE_SETS)
    cs = {n for _, k, _, n in all_runs(recs) if k == "E"}
    cg = collections.defaultdict(set)
    for r in recs:
        for n, c in r.cigar:
            cg[c].add(n)
    steps = {9, 10, 99, 100, 999, 1000, 9999, 10000}
    assert steps <= cs, sorted(steps - cs)
    assert steps <= cg["M"], sorted(steps - cg["M"])
    for c in "ID":
        assert {9, 10, 99, 100} <= cg[c], (c, sorted(cg[c]))
    assert any(1000 <= n <= 9999 for n in cg["D"]) and any(n >= 10000 for n in cg["D"]), "a deletion run of four digits, and one of five"
    assert {1, 2, 3, 4, 5} == {len(str(n)) for n in cs}


def test_ends(sets):
    recs = records(sets, "drb5-edges")
    first = collections.defaultdict(list)
    last = collections.defaultdict(list)
    for r in recs:
        first[r.cols[0][0]].append(r)
        last[r.cols[-1][0]].append(r)
    assert first["D"] and first["E"] and set(last) >= set("IDXE"), (sorted(first), sorted(last))
    # a leading insertion: the read has nothing of the graph before it
    assert any(r.path_start == 0 and r.cols[0][0] == "I" for r in recs)
    assert pileup_ref.walk(sets["drb5-edges"].gaf, *_arrays(sets["drb5-edges"])[:2])[2] >= 1
    # (and on DRB1, whose pileup lists k_pu_events writes itself)
    assert any(r.path_start == 0 and r.cols[0][0] == "I" for r in records(sets, "drb1-runs"))
    assert pileup_ref.walk(sets["drb1-runs"].gaf, *_arrays(sets["drb1-runs"])[:2])[2] >= 1


def test_letters(sets):
    recs = records(sets, "drb5-edges")
    n_cols = [(r, f) for r in recs for f, (k, _, q) in enumerate(r.cols) if q == "n"]
    assert any(r.cols[f][0] == "X" for r, f in n_cols), "N in a mismatch"
    assert any(r.cols[f][0] == "I" for r, f in n_cols), "N in an insertion"
    assert {0, 63} <= {f % 64 for r, f in n_cols if r.cols[f][0] == "X"}, "N as the read base of a mismatch at lane 0 and at lane 63"
    # (and in the sweep set, whose pileup lists k_pu_events writes itself)
    assert {0, 63} <= {f % 64 for r in records(sets, "drb1-sweep") for f, (k, _, q) in enumerate(r.cols) if k == "X" and q == "n"}


ENTRIES_IN_A_BLOCK = 40  # the most the oracle shows on DRB1: 40 of 64 operations enter a node (one-base nodes in runs)


def test_node_entries(sets):
    most = max(max(collections.Counter(f // 64 for f, _, _ in r.entries).values()) for r in records(sets, "drb1-entries"))
    assert most == ENTRIES_IN_A_BLOCK >= 32, most
    for name in ("drb1-sweep", "synth-nodes"):
        recs = records(sets, name)
        by_d = only_d = 0
        cont = set()
        for r in recs:
            for (f, _, adjacent), nxt in zip(r.entries, r.entries[1:] + [(len(r.cols), 0, False)]):
                by_d += r.cols[f][0] == "D"
                only_d += all(r.cols[g][0] in "DI" for g in range(f, nxt[0])) and r.cols[f][0] == "D"
                if f % 64 == 0 and f and r.cols[f][0] == "E" and r.cols[f - 1][0] == "E":
                    cont.add(adjacent)
        assert by_d and only_d, (name, "a node entered by a deletion, a node crossed by deleted bases only")
        assert cont == {True, False}, (name, "a node entered at lane 0 inside an = run, graph-adjacent and not", cont)


def _arrays(s):
    a = oracle_index_arrays(s.index)
    return a["node_seq_idx"], a["seq_fwd"], a["node_edge_idx"], a["node_edges_to"], a["edges"]


def test_reference_walkers_agree(sets):
    for name, s in sets.items():
        idx, seq, eidx, eto, edges = _arrays(s)
        counts, n_al, _ = pileup_ref.walk(s.gaf, idx, seq)
        base, node, _, n_cov = coverage_ref.walk(s.gaf, idx, eidx, eto, edges)
        assert n_al == n_cov == len(s.case.reads), name
        assert np.array_equal(counts[:, :5].sum(1, dtype=np.uint32), base), name
        assert int(node.sum()) == sum(len(r.path) for r in s.records), name
        assert int(counts[:, pileup_ref.DEL].sum()) == sum(k == "D" for r in s.records for k, _, _ in r.cols), name


def test_both_strands_set(sets):
    c = sets["drb1-both-strands"].case
    assert c.both_strands and [n for n, s in sets.items() if s.case.both_strands] == ["drb1-both-strands"]
    fwd = M.forward_reads(c)
    assert [a != b for a, b in zip(c.reads, fwd)] == [bool(i % 2) for i in range(len(fwd))]
    assert all(M.rc(a) == b for a, b in zip(c.reads[1::2], fwd[1::2]))
