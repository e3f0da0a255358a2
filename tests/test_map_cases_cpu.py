"""tests/map_cases.py produces what it is there for -- judged from the oracle alone, so that tests/test_map_cases_gpu.py cannot
pass vacuously: score ties at most steps of a repeat's DP, the listed anchor counts, a jump across exactly max_gap and none
across max_gap + 1, an anchor that ends on the last base of a graph of 2^n bases, reads on both sides of the integer-argmax
threshold, several chains on one maximum, strand ties."""
import ctypes as C

import pytest

import map_cases as M


@pytest.fixture(scope="module")
def chained(oracle):
    """(case, read number) -> the oracle's ChainResult under the case's parameters; indexes and results are built once"""
    indexes, results = {}, {}

    def index(case):
        key = (tuple(case.nodes), case.k)
        if key not in indexes:
            indexes[key] = oracle.Index(oracle.Graph.from_nodes_edges(case.nodes, case.edges), case.k)
        return indexes[key]

    def run(case, r, seq=None):
        p = M.params_of(case)
        s = case.reads[r] if seq is None else seq
        key = (tuple(case.nodes), case.k, s, p["bandwidth"], p["max_gap"], p["chain_min_n_anchors"], p["only_forward"])
        if key not in results:
            results[key] = oracle.chain_anchors(index(case), s, p["bandwidth"], p["max_gap"], p["chain_min_n_anchors"],
                                                only_forward=bool(p["only_forward"]))
        return results[key]

    run.index = index
    return run


def case(name):
    return next(c for c in M.all_cases() if c.name == name)


def real_chains(res):
    return [ch for ph, ch in zip(res.is_placeholder, res.chains) if not ph]


def only_placeholder(res):
    return res.is_placeholder == [True]


def test_cases_are_well_formed():
    cs = M.all_cases()
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        assert [i for i, _ in c.nodes] == list(range(1, len(c.nodes) + 1)), c.name
        assert all(s and set(s) <= set("ACGT") for _, s in c.nodes), c.name
        assert c.edges == [(i, i + 1) for i in range(1, len(c.nodes))] or c.name.startswith("equal-shared-predecessor"), c.name
        assert set(c.params) <= set(M.DEFAULTS), c.name
        assert 1 <= len(c.reads) <= 300
    assert {c.family for c in cs} == {"repeat", "count", "gap", "sort", "argmax", "equal", "strand"}


# ---------------------------------------------------------------- a
def tied_steps(oracle, res, k, bandwidth, max_gap):
    """(steps whose best window score is held by two or more predecessors, steps): og_score_anchor over the sorted anchors,
    which carry their final f(j) -- what the DP saw when it scored them as predecessors"""
    sa = res.sorted_anchors
    arr = (oracle.Anchor * len(sa))(*[oracle.Anchor(x.id, x.query_begin, x.query_end, oracle.SeqPos(*x.target_begin),
                                                    oracle.SeqPos(*x.target_end), x.max_chain_score, x.best_predecessor_id) for x in sa])
    score, ref = oracle.lib().og_score_anchor, [C.byref(a) for a in arr]
    tied = 0
    for i in range(1, len(sa)):
        s = [score(ref[j], ref[i], k, max_gap) for j in range(max(0, i - bandwidth), i)]
        best = max(s)
        tied += best > -1.0e300 and s.count(best) >= 2
    return tied, len(sa) - 1


@pytest.mark.parametrize("name", [c.name for c in M.cases("repeat") if c.params["chain_min_n_anchors"] == 1])
def test_repeat_reads_tie_at_most_steps(oracle, chained, name):
    """the argmax rule `largest j among the lanes that hold the maximum` decides a step only when the maximum is shared: at least
    half of the steps of the read that is the repeat once (ties do not depend on chain_min_n_anchors)"""
    c = case(name)
    p = M.params_of(c)
    tied, steps = tied_steps(oracle, chained(c, 0), c.k, p["bandwidth"], p["max_gap"])
    print(name, "tied steps", tied, "of", steps)
    assert steps > 0 and 2 * tied >= steps


def test_repeats_give_several_chains_and_bare_placeholders(chained):
    several, placeholders = [], []
    for c in M.cases("repeat"):
        for r in range(len(c.reads)):
            res = chained(c, r)
            if len(real_chains(res)) > 1:
                several.append((c.name, r))
            if only_placeholder(res):
                placeholders.append((c.name, r))
    assert several and placeholders
    # A x 90 on A x 30: 80 anchors end on every target position, the 50 predecessors of the window end where the anchor ends
    for name in ("repeat-Ax30-fwd-min1", "repeat-Ax30-fwd-min3", "repeat-Ax30-all-min1"):
        assert (name, 1) in placeholders
    # AT x 20 with both orientations: every record twice, once per strand
    assert len(chained(case("repeat-ATx20-all-min1"), 0).sorted_anchors) == 2 * M.forward_anchor_count(case("repeat-ATx20-all-min1"), "AT" * 20)
    assert any(x.target_end[0] for x in chained(case("repeat-ATx20-all-min1"), 0).sorted_anchors)


# ---------------------------------------------------------------- b
@pytest.mark.parametrize("name", [c.name for c in M.cases("count")])
def test_anchor_counts_are_the_listed_ones(chained, name):
    c = case(name)
    n = len(M.ANCHOR_COUNTS)
    assert [len(chained(c, r).sorted_anchors) for r in range(n)] == list(M.ANCHOR_COUNTS)
    assert [M.forward_anchor_count(c, s) for s in c.reads[:n]] == list(M.ANCHOR_COUNTS)
    ma = M.params_of(c)["chain_min_n_anchors"]
    for r, a in enumerate(M.ANCHOR_COUNTS):
        clean, sub = chained(c, r), chained(c, n + r)
        if a >= 63:
            assert [len(ch) for ch in real_chains(clean)] == [a]
            # two substitutions cost the k-mers over them; one chain still holds every anchor left: it jumped twice
            assert len(sub.sorted_anchors) == a - 2 * c.k
            assert [len(ch) for ch in real_chains(sub)] == [a - 2 * c.k]
        else:
            assert len(sub.sorted_anchors) == 0 and only_placeholder(sub)
    # the read of two anchors: a chain of two, rolled back when three are asked for
    two = chained(c, M.ANCHOR_COUNTS.index(2))
    assert two.curr_max == c.k + 1.0
    assert ([len(ch) for ch in real_chains(two)] == [2]) if ma <= 2 else only_placeholder(two)
    assert only_placeholder(chained(c, 0))


# ---------------------------------------------------------------- c
def jumps_from_x_to_z(c, res):
    """anchors that begin in Z and whose best predecessor ends in X"""
    x_len, z_begin = len(c.nodes[0][1]), len(M.linear_sequence(c)) - len(c.nodes[-1][1])
    end_of = {a.id: a.target_end[1] for a in res.sorted_anchors}
    return [a for a in res.sorted_anchors
            if a.target_begin[1] >= z_begin and a.best_predecessor_id >= 0 and end_of[a.best_predecessor_id] <= x_len]


@pytest.mark.parametrize("name", [c.name for c in M.cases("gap")])
def test_gap_of_max_gap_is_jumped_and_one_more_is_not(chained, name):
    c = case(name)
    mg = M.params_of(c)["max_gap"]
    ylen = len(M.linear_sequence(c)) - 800
    assert len(c.nodes) == (3 if ylen else 2) and len(c.nodes[0][1]) == len(c.nodes[-1][1]) == 400
    res = chained(c, 0)
    assert len(res.sorted_anchors) == (790 if ylen == 0 else 780)
    jumps = jumps_from_x_to_z(c, res)
    if ylen == 0:  # no Y: the read is the graph, one chain over the junction's k-mers
        assert [len(ch) for ch in real_chains(res)] == [800 - c.k + 1]
    elif ylen <= mg:
        assert jumps and len(real_chains(res)) == 1
        if ylen == mg:  # the jump pays the table's last entry
            j = jumps[0]
            pred = next(a for a in res.sorted_anchors if a.id == j.best_predecessor_id)
            assert (j.target_begin[1] - pred.target_begin[1]) - (j.query_begin - pred.query_begin) == mg
    else:
        assert ylen == mg + 1 and not jumps
        chains = real_chains(res)
        assert len(chains) == 2 and chains[0][-1].max_chain_score == chains[1][-1].max_chain_score == res.curr_max


# ---------------------------------------------------------------- d
@pytest.mark.parametrize("name", [c.name for c in M.cases("sort")])
def test_an_anchor_ends_on_the_last_base(chained, name):
    c = case(name)
    L = int(name.split("L")[1])
    assert chained.index(c).seq_length == L
    assert max(a.target_end[1] for a in chained(c, 0).sorted_anchors) == L
    one = chained(c, 1).sorted_anchors
    assert len(one) == 1 and one[0].target_end == (0, L)
    assert len(chained(c, 0).sorted_anchors) == len(chained(c, 2).sorted_anchors) == 30


# ---------------------------------------------------------------- e
def test_reads_on_both_sides_of_the_integer_argmax_threshold(chained):
    c = M.argmax_case()
    limit = M.key_anchors(c.k, M.params_of(c)["max_gap"])
    assert limit == 25160
    counts = [len(chained(c, r).sorted_anchors) for r in range(len(c.reads))]
    print("anchors", counts, "threshold", limit)
    assert counts == [M.forward_anchor_count(c, s) for s in c.reads]
    sides = M.argmax_sides(c)
    assert sides == [n > limit for n in counts] and sides == [False, True, False, True, False, False]
    assert 10500 < counts[0] < 11500 and 28500 < counts[1] < 29500 and 33500 < counts[3] < 34500
    # every workgroup (four reads) of the launch holds both kinds
    assert any(sides[:4]) and not all(sides[:4])


# ---------------------------------------------------------------- f
def test_equal_chains_and_consumed_anchors(chained):
    c = M.equal_chain_case()
    res = chained(c, 0)
    chains = real_chains(res)
    assert len(chains) >= 2 and all(ch[-1].max_chain_score == res.curr_max for ch in chains)


def on_the_maximum(res):
    return [a for a in res.sorted_anchors if a.max_chain_score == res.curr_max and a.best_predecessor_id >= 0]


@pytest.mark.parametrize("ma", M.MIN_ANCHORS)
def test_two_anchors_on_the_maximum_share_their_predecessor(chained, ma):
    c = case("equal-shared-predecessor-min%d" % ma)
    for r in (0, 1):
        res = chained(c, r)
        tops = on_the_maximum(res)
        assert len(tops) == 2 and tops[0].best_predecessor_id == tops[1].best_predecessor_id
        assert tops[0].target_begin == tops[1].target_begin and tops[0].target_end != tops[1].target_end
        n = len(c.reads[r]) - c.k + 1
        # the second chain ends on the anchor the first one consumed: two anchors, below a minimum of three
        assert [len(ch) for ch in real_chains(res)] == ([n, 2] if ma <= 2 else [n])
    assert len(on_the_maximum(chained(c, 2))) == 1


# ---------------------------------------------------------------- g
def test_strand_ties_are_exact(chained):
    import numpy as np

    c = M.strand_case()
    for r in M.STRAND_TIE_READS:
        f, b = chained(c, r), chained(c, r, M.rc(c.reads[r]))
        assert real_chains(f) and real_chains(b)
        assert np.float64(f.curr_max).view(np.uint64) == np.float64(b.curr_max).view(np.uint64) and f.curr_max > 0.0
    assert c.reads[2] == M.rc(c.reads[2]) and c.reads[0] == M.rc(c.reads[1])
    f, b = chained(c, 3), chained(c, 3, M.rc(c.reads[3]))
    assert only_placeholder(f) and real_chains(b)
