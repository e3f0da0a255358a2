"""tests/sg_cases.py reaches what it is there for, shown from the oracle alone (no GPU): every cell of every family has its
cases, the restated extension walk yields exactly the oracle's range on every case, the reference's rows add up to the oracle's
poa_rows, no head or tail of junk anchors, and every read is aligned.  The tables are printed (pytest -s shows them)."""
import pytest

import sg_cases as S


@pytest.fixture(scope="module")
def world(oracle):
    spec, marks, cases = S.all_cases()
    ix = oracle.Index(S.make_graph(oracle, spec), S.K)
    view = S.IndexView(ix)
    facts, anchors = [], []
    for c in cases:
        f, res = S.facts_of(oracle, ix, view, spec, c)
        facts.append(f)
        anchors.append(res.sorted_anchors)
    return spec, cases, ix, view, facts, anchors


def test_the_set_is_small_and_has_topological_ids(world):
    spec, cases, _, _, _, _ = world
    assert len(spec.nodes) <= 2250 and max(len(c.read.seq) for c in cases) <= 6000
    assert len(cases) >= 40 and len({c.name for c in cases}) == len(cases)
    assert {c.family for c in cases} == set(S.FAMILIES)
    # an edge between forward strands leads to a larger id; the two links into a reverse strand are the strand family's
    assert all(a < b for a, b in spec.edges if not (a | b) & 1)
    assert sum(1 for a, b in spec.edges if (a | b) & 1) == 2


@pytest.mark.parametrize("fam", S.FAMILIES)
def test_every_cell_of_the_family_is_reached(world, fam):
    facts = world[4]
    rows = S.table(facts, fam)
    print("\n%s" % fam)
    for cell, need, hit, differ in rows:
        print("  %-66s %2d case(s): %s%s" % (cell, len(hit), ", ".join(hit[:5]) + (" ..." if len(hit) > 5 else ""),
                                           "   [remain rules differ on %d]" % len(differ) if cell in S.RULE_SENSITIVE else ""))
    empty = [cell for cell, need, hit, _ in rows if len(hit) < need]
    assert not empty, empty
    # a family's own cases reach its cells (other families' cases only add to them)
    own = S.table([f for f in facts if f.case.family == fam], fam)
    if fam != "gap":  # (the unconnected nodes inside a range are those of the pass and group reads)
        assert not [cell for cell, need, hit, _ in own if len(hit) < need]
    blind = [cell for cell, _, _, differ in rows if cell in S.RULE_SENSITIVE and not differ]
    assert not blind, blind


def test_the_restated_walk_yields_the_oracle_range(world):
    """the claim in the header of csrc/vga_subgraph.hip: a handle is in the range iff it can be reached with a positive budget,
    expanding only while length < budget -- on fans, diamonds, strand links and budgets of 0 and 1"""
    _, _, _, view, facts, _ = world
    walked = 0
    for f in facts:
        hs, up, down = S.extension(view, f.desc)
        assert hs == f.sub.range_handles, f.case.name
        assert all(b > 0 for b in list(up.values()) + list(down.values()))
        walked += bool(up) + bool(down)
    assert walked >= 30


def test_reference_rows_add_up_to_the_oracle_poa_rows_and_every_read_aligns(oracle, world):
    _, cases, ix, _, facts, _ = world
    for rule in (S.LONGEST_PATH, S.FIRST_EDGE):
        mp = oracle.default_map_params()
        mp.poa.remain_rule = rule
        _, ag, st = oracle.map_reads(ix, [c.name for c in cases], [c.read.seq for c in cases], mp)
        lines = ag.splitlines()
        assert len(lines) == len(cases)
        assert not [ln.split("\t")[0] for ln in lines if ln.split("\t")[5] == "*"]
        assert st["poa_rows"] == sum(f.ref[rule]["N"] for f in facts)
        assert st["n_aligned_reads"] == len(cases)


def test_no_head_or_tail_anchors(world):
    _, cases, _, _, facts, anchors = world
    for c, f, an in zip(cases, facts, anchors):
        rd = c.read
        assert an, c.name
        assert all(a.query_begin >= rd.head and a.query_end <= len(rd.seq) - rd.tail for a in an), c.name
        # ... so a budget is never more than the junk (the last node in front of 130 arms has no k-mers of its own -- the
        # index leaves out a node of more than 100 neighbours -- and its bases take that part of the tail's budget back)
        assert f.desc["q_first"] >= rd.head and f.prefix <= rd.head and f.suffix <= rd.tail, c.name


def test_reference_is_consistent_with_itself(world):
    """cheap cross-checks of the reference's own fields against each other: counts against list lengths, sinks against flags,
    predecessor words against the list"""
    for f in world[4]:
        for rule, r in f.ref.items():
            t = r["table"][1:]
            assert r["n_nodes"] == len(t) == len(r["handles"]) == len(r["first_row"])
            assert r["N"] == len(r["seq"]) == sum(x[1] for x in t)
            assert r["n_preds"] == len(r["preds"]) == sum(x[2] for x in t)
            assert r["n_sinks"] == len(r["sinks"]) == sum(x[3] for x in t)
            assert r["sinks"] == [x[0] + x[1] - 1 for x in t if x[3]]
            for x in t:
                assert (x[6] == 0 or x[6] in r["preds"]) if x[2] == 1 else r["preds"][x[6]:x[6] + x[2]] == sorted(r["preds"][x[6]:x[6] + x[2]])
            assert all(x[5] == 0 for x in t if x[3]) and r["table"][0][5] == r["longest"] <= r["N"]
        a, b = f.ref[S.LONGEST_PATH], f.ref[S.FIRST_EDGE]
        assert all(x[5] >= y[5] for x, y in zip(a["table"], b["table"]))
        assert {k: v for k, v in a.items() if k not in ("table", "longest")} == {k: v for k, v in b.items() if k not in ("table", "longest")}
