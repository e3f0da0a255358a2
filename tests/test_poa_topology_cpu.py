"""The POA problems of tests/poa_topologies.py on the CPU: (1) the fixed set the GPU tests run reaches, judged from the oracle's
results alone, every branch it is there for -- a condition on the fixtures: no cell may be empty; (2) the oracle is the true
optimum on small members of every family, against the path-enumerating general-gap programme of test_oracle_poa_cpu.py;
(3) the adaptive band does not move the optimum of low-error reads on them."""
import os
import random
import re

import pytest

import poa_topologies as T
from helpers import ROOT
from test_oracle_poa_cpu import all_paths, wsb_global

PENS = [(2, 4, 4, 2, 24, 1), (1, 3, 2, 2, 10, 1), (2, 2, 1, 3, 6, 1)]  # the three of test_oracle_poa_cpu.py


@pytest.fixture(scope="module")
def refs(oracle):
    """oracle results of the fixed set under the default parameters"""
    return [oracle.poa_align(*c.problem) for c in T.fixed_set()]


def test_generators_are_seeded_and_well_formed():
    a, b = T.fixed_set(), T.fan_cases() + T.reach_cases() + T.source_sink_cases() + T.rand_dag_cases()
    assert [c.problem for c in a] == [c.problem for c in b]
    assert len({c.name for c in a}) == len(a)
    for c in a:
        nodes, edges, q = c.problem
        assert q and all(nodes) and all(0 <= s < d < len(nodes) for s, d in edges) and len(set(edges)) == len(edges), c.name
    fans = {int(re.match(r"fan(\d+)-", c.name).group(1)) for c in a if re.match(r"fan\d+-(equal|unequal)", c.name)}
    assert fans == set(T.FAN_ARMS)
    deg = max(max(len(p) for p in T.pred_lists(len(c.problem[0]), c.problem[1])) for c in a if c.family == "dag")
    reach = max(d - s for c in a if c.family == "dag" for s, d in c.problem[1])
    assert 9 <= deg <= 12 and 70 <= reach <= 80, (deg, reach)


def test_classify_on_a_hand_made_result():
    """three predecessors; the path enters node 4 from node 2 (position 1 of [1, 2, 3]) with a 2-base deletion, 20 ties"""
    from collections import namedtuple
    R = namedtuple("R", "cigar graph_nodes")
    nodes, edges = ["AC", "G", "T", "A", "CCGT"], [(0, 1), (0, 2), (0, 3), (1, 4), (2, 4), (3, 4)]
    assert T.classify(nodes, edges, R("3M2D1I2M", [0, 0, 2, 4, 4, 4, 4])) == [(4, 3, 1, "short")]
    assert T.classify(nodes, edges, R("2M1D1M1I3M", [0, 0, 3, 4, 4, 4, 4])) == [(4, 3, 2, "match")]
    assert [T.deletion_piece(k) for k in (1, 19, 20, 21, 35)] == ["short", "short", "tie", "long", "long"]
    assert T.deletion_piece(9, (1, 3, 2, 2, 10, 1)) == "long"
    assert T.far_nodes_on_path(nodes, edges, R("3M2D1I2M", [0, 0, 2, 4, 4, 4, 4])) == [(0, 3, False), (2, 2, True)]


def test_fixed_set_enters_joins_at_every_position_class_with_every_operation(refs):
    cells = {}
    for c, r in zip(T.fixed_set(), refs):
        assert r.ok, c.name
        for v, deg, pos, op in T.classify(c.problem[0], c.problem[1], r):
            cls = ["<4" if pos < 4 else "=4" if pos == 4 else ">4"] + (["last of 255"] if deg == 255 and pos == 254 else [])
            for k in cls:
                cells.setdefault((k, op), []).append(c.name)
    for k in ("<4", "=4", ">4", "last of 255"):
        for op in ("match", "short", "long"):
            assert cells.get((k, op)), f"no problem of the fixed set enters a join at position {k} with a {op}"
    print({k: len(v) for k, v in sorted(cells.items())})


def test_fixed_set_has_reach_32_and_33_on_the_path_taken_and_walked(refs):
    seen = set()
    for c, r in zip(T.fixed_set(), refs):
        seen |= {(reach, far) for _, reach, far in T.far_nodes_on_path(c.problem[0], c.problem[1], r)}
    for reach in (31, T.RING_SPAN, T.RING_SPAN + 1, 64, 200):
        assert (reach, True) in seen and (reach, False) in seen, reach
    assert max(x for x, far in seen if far) >= 400  # the row that outlives a dozen turns of the ring


def test_fixed_set_has_an_optimal_source_that_is_not_the_first_and_sink_that_is_not_the_last(refs):
    both = []
    for c, r in zip(T.fixed_set(), refs):
        if c.family != "srcsink":
            continue
        nodes, edges, _ = c.problem
        srcs = [v for v in range(len(nodes)) if all(d != v for _, d in edges)]
        snks = [v for v in range(len(nodes)) if all(s != v for s, _ in edges)]
        first, last = r.graph_nodes[0], r.graph_nodes[-1]
        assert first in srcs and last in snks
        longest = max(snks, key=lambda v: len(nodes[v]))
        if len(srcs) > 1 and first != srcs[0] and last not in (snks[-1], longest):
            both.append(c.name)
    assert both
    assert {len([1 for c in T.fixed_set() if c.name.startswith(f"src{n}-")]) > 0 for n in (1, 2, 3, 5, 8)} == {True}


def test_wide_estimate_problems_keep_a_launch_from_the_one_wave_kernel(oracle):
    """the width estimate of poa_call::est_width (csrc/vga_poa_run.hip) restated: beyond 1 000 columns poa_choose_shape leaves
    k_poa_dp_t6 out, which is what lets VGA_POA_KERNEL=t7 reach k_poa_dp_t7 with small problems.  Their paths enter the join at
    positions 4 and 5 by a match, a short and a long deletion."""
    seen = set()
    for c in T.wide_estimate_cases():
        nodes, edges, q = c.problem
        longest = len(nodes[0]) + max(len(nodes[v]) for v in range(1, 7)) + len(nodes[7]) + len(nodes[8])
        assert edges[0] == (0, 1) and len(nodes[1]) == 3200  # the first out-edge and the longest path agree: either remain rule
        w = 10 + int(0.01 * len(q))
        assert min(len(q) + 1, 2 * w + 431 + 0.3 * abs(longest - len(q))) > 1000
        r = oracle.poa_align(nodes, edges, q)
        assert r.ok
        seen |= {(pos, op) for _, _, pos, op in T.classify(nodes, edges, r)}
    assert seen == {(p, op) for p in (4, 5) for op in ("match", "short", "long")}


def test_ring_span_is_one_number():
    """the threshold between ring rows and kept rows is written in the POA host code, in the device subgraph builder and in
    the generators: the three agree"""
    csrc = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
    poa = re.search(r"#define\s+POA_RING_SPAN\s+(\d+)", open(os.path.join(csrc, "vga_poa_launch.hpp")).read())
    sg = re.search(r"#define\s+SG_RING_SPAN\s+(\d+)u?\b", open(os.path.join(csrc, "vga_subgraph.hip")).read())
    assert int(poa.group(1)) == int(sg.group(1)) == T.RING_SPAN


# ---------------------------------------------------------------- the oracle is the optimum on these shapes
def small_members(rng):
    """(nodes, edges, query) with few enough source-to-sink paths to enumerate"""
    out = []
    for n in (2, 5, 9, 17, 40):  # fan-in, arms of 1-5 bases
        nodes, edges, arms = T.fan_graph(rng, [rng.randint(1, 5) for _ in range(n)], join_len=6, order=rng.choice(("fwd", "rev")))
        nodes[0], nodes[-1] = nodes[0][:4], nodes[-1][:3]
        for kind in ("clean", "del2", "ins"):
            out.append((nodes, edges, T.fan_query(rng, nodes, arms, rng.randrange(n), kind)))
        out.append((nodes, edges, T._seq(rng, rng.randint(3, 14))))
    nodes, edges, arms = T.fan_graph(rng, [2, 3, 1, 4, 2, 3], join_len=30, chain_arms=True)
    nodes[0], nodes[-1] = nodes[0][:3], nodes[-1][:3]
    out.append((nodes, edges, T.fan_query(rng, nodes, arms, 4, "del" + str(rng.randint(21, 25)))))  # second gap piece over a join
    for r in (33, 36, 40):  # reach beyond the ring, one-base nodes
        skips = [(2, 2 + r), (3, 20), (10, 3 + r)]
        nodes, edges = T.chain_graph(rng, r + 6, skips, far_first=rng.random() < 0.5, lo=1, hi=1)
        for taken in ([], skips[:1], skips[2:], [(3, 20)]):
            out.append((nodes, edges, T.chain_query(rng, nodes, taken, 0.05)))
    nodes, edges = T.source_sink_graph(rng, 3, 3)  # 3 sources x 3 sinks
    nodes = [s[:rng.randint(1, 7)] for s in nodes]
    for s in range(3):
        for k in range(3):
            q = nodes[s] + nodes[3] + nodes[4 + k]
            out.append((nodes, edges, "".join(c if rng.random() > 0.1 else rng.choice("ACGT") for c in q)))
    return out


@pytest.mark.parametrize("pen", PENS)
def test_oracle_score_is_the_optimum_on_fans_far_edges_and_several_sources_and_sinks(oracle, pen):
    m, x, o1, e1, o2, e2 = pen
    g = lambda k: min(o1 + k * e1, o2 + k * e2)
    p = oracle.default_poa_params()
    p.match, p.mismatch, p.gap_open1, p.gap_ext1, p.gap_open2, p.gap_ext2 = pen
    p.wb = -1  # no band: the oracle must find the global optimum
    problems = small_members(random.Random(PENS.index(pen) + 11))
    assert len(problems) == 42
    cache = {}
    for nodes, edges, q in problems:
        paths = all_paths(len(nodes), edges)
        assert len(paths) <= 40
        want = -10**9
        for path in paths:
            s = "".join(nodes[v] for v in path)
            if (s, q) not in cache:
                cache[(s, q)] = wsb_global(s, q, m, x, g)
            want = max(want, cache[(s, q)])
        for rule in (0, 1):  # without a band the remain rule moves nothing
            p.remain_rule = rule
            r = oracle.poa_align(nodes, edges, q, p)
            assert r.ok and r.best_score == want, (nodes, edges, q, r.best_score, want, r.cigar)


def test_banded_oracle_equals_unbanded_on_low_error_reads_of_fans_and_far_edges(oracle):
    """the adaptive band (b = 10, f = 0.01) is wide enough for a low-error read that follows equal arms or a chain, whichever
    arm or skip edge it takes: same optimum as without a band, under both remain rules"""
    rng = random.Random(8)
    problems = []
    for n in (5, 17, 64):
        nodes, edges, arms = T.fan_graph(rng, [12] * n, join_len=40)
        problems += [(nodes, edges, T.fan_query(rng, nodes, arms, pos, kind)) for pos in T.fan_positions(n) for kind in ("clean", "del2", "ins")]
    for r in (32, 33, 64):
        nodes, edges = T.chain_graph(rng, r + 14, [(6, 6 + r)])
        problems += [(nodes, edges, T.chain_query(rng, nodes, taken, 0.03)) for taken in ([], [(6, 6 + r)])]
    for rule in (0, 1):
        pb, pu = oracle.default_poa_params(), oracle.default_poa_params()
        pu.wb = -1
        pb.remain_rule = pu.remain_rule = rule
        for nodes, edges, q in problems:
            b, u = oracle.poa_align(nodes, edges, q, pb), oracle.poa_align(nodes, edges, q, pu)
            assert b.ok and u.ok and b.best_score == u.best_score, (rule, len(nodes), q)
