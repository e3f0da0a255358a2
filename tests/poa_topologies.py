"""Seeded POA problems of the graph shapes `_rand_problem` (tests/test_gpu_parity.py) never draws: joins of more than four
predecessors, value rows read more than POA_RING_SPAN (32) nodes ahead, several sources and sinks.  Plain Python: no GPU, no
oracle.  A problem is `(nodes, edges, query)` as `Context.poa_batch` and `oracle.poa_align` take it; nodes are in topological
order and edges in edge-list order -- that order is the order of a node's predecessor list and names its first out-edge.

`fixed_set()` is the set the GPU tests run (tests/test_poa_topology_gpu.py); tests/test_poa_topology_cpu.py holds it to the
coverage it has to have, judged from the oracle's results with `classify` / `far_nodes_on_path`."""
import random
from collections import namedtuple

DEFAULT_PEN = (2, 4, 4, 2, 24, 1)  # match, mismatch, open1, ext1, open2, ext2 (oracle/og_poa.c)
RING_SPAN = 32                     # POA_RING_SPAN (csrc/vga_poa_launch.hpp): a node read further ahead keeps its value row
FAN_ARMS = (2, 4, 5, 8, 17, 64, 255)
UNEQUAL = (1, 2, 5, 40, 400)
ENTRIES = ("clean", "del1", "del2", "del3", "del35", "ins")

Case = namedtuple("Case", "name family problem")


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _other(rng, c):
    return rng.choice([x for x in "ACGT" if x != c])


def _enter(rng, kind, join):
    """the query's bases for a join node entered in the given way"""
    if kind == "clean":
        return join
    if kind == "ins":
        return _seq(rng, 3) + join
    return join[int(kind[3:]):]  # del<k>: the first k bases of the join are not in the read


# ---------------------------------------------------------------- fan-in
def fan_graph(rng, arm_lens, join_len=90, order="fwd", chain_arms=False):
    """head -> len(arm_lens) arms -> join -> tail.  Returns (nodes, edges, arms): arms[i] is the list of nodes of arm i, and
    arm i is at position i of the join's predecessor list (order="rev": at position n - 1 - i)."""
    n = len(arm_lens)
    nodes, edges, arms = [_seq(rng, 30)], [], []
    for ln in arm_lens:
        if chain_arms:
            a = len(nodes)
            nodes += [_seq(rng, ln), _seq(rng, max(1, ln // 2))]
            arms.append([a, a + 1])
        else:
            arms.append([len(nodes)])
            nodes.append(_seq(rng, ln))
    join = len(nodes)
    nodes += [_seq(rng, join_len), _seq(rng, 30)]
    for a in arms:
        edges.append((0, a[0]))
    for a in arms:
        if len(a) == 2:
            edges.append((a[0], a[1]))
    for a in (arms if order == "fwd" else arms[::-1]):
        edges.append((a[-1], join))
    edges.append((join, join + 1))
    return nodes, edges, arms


def fan_query(rng, nodes, arms, arm, kind):
    join = arms[-1][-1] + 1
    return nodes[0] + "".join(nodes[v] for v in arms[arm]) + _enter(rng, kind, nodes[join]) + nodes[join + 1]


def fan_positions(n):
    return sorted({p for p in (0, 3, 4, 5, n - 1) if p < n})


def fan_cases(seed=2024):
    out = []
    for n in FAN_ARMS:
        rng = random.Random(seed * 1000 + n)
        # equal arms: every followed arm with every way into the join
        for order in ("fwd", "rev") if n in (5, 8) else ("fwd",):
            nodes, edges, arms = fan_graph(rng, [12] * n, order=order)
            for pos in fan_positions(n):
                arm = pos if order == "fwd" else n - 1 - pos
                for kind in ENTRIES:
                    out.append(Case(f"fan{n}-equal-{order}-p{pos}-{kind}", "fan", (nodes, edges, fan_query(rng, nodes, arms, arm, kind))))
        # wildly unequal arms: the predecessor rows' bands barely overlap the cell, or miss it
        lens = [UNEQUAL[(i + n) % 5] for i in range(n)]
        nodes, edges, arms = fan_graph(rng, lens)
        for k, pos in enumerate(fan_positions(n)):
            for kind in ("clean", ENTRIES[1 + (k + n) % 5]):
                out.append(Case(f"fan{n}-unequal-p{pos}-{kind}", "fan", (nodes, edges, fan_query(rng, nodes, arms, pos, kind))))
    rng = random.Random(seed + 1)
    # arms that are two-node chains
    nodes, edges, arms = fan_graph(rng, [6 + i for i in range(7)], chain_arms=True)
    for pos in (0, 4, 6):
        for kind in ("clean", "del2", "del35"):
            out.append(Case(f"fan7-chains-p{pos}-{kind}", "fan", (nodes, edges, fan_query(rng, nodes, arms, pos, kind))))
    # fan -> fan: the tail of the first is the head of the second
    for n1, n2 in ((5, 6), (9, 3)):
        a_nodes, a_edges, a_arms = fan_graph(rng, [10] * n1)
        b_nodes, b_edges, b_arms = fan_graph(rng, [3 + 2 * i for i in range(n2)])
        sh = len(a_nodes) - 1
        nodes = a_nodes + b_nodes[1:]
        edges = a_edges + [(s + sh, d + sh) for s, d in b_edges]
        ja, jb = a_arms[-1][-1] + 1, b_arms[-1][-1] + 1
        for p1, p2, k1, k2 in ((n1 - 1, n2 - 1, "clean", "del1"), (4, 0, "del35", "clean"), (0, 2, "ins", "del35"), (4, n2 - 1, "del3", "ins")):
            q = (a_nodes[0] + a_nodes[a_arms[p1][0]] + _enter(rng, k1, a_nodes[ja]) + a_nodes[ja + 1]
                 + b_nodes[b_arms[p2][0]] + _enter(rng, k2, b_nodes[jb]) + b_nodes[jb + 1])
            out.append(Case(f"fan{n1}-fan{n2}-p{p1}{k1}-p{p2}{k2}", "fan", (nodes, edges, q)))
    return out


def wide_estimate_cases(seed=41):
    """A fan of 6 arms behind a 1 100-base head whose first arm has 3 200 bases, followed along arms 4 and 5.  The band stays
    narrow, but the library's estimate of a problem's widest row -- min(qlen + 1, 2 w + 431 + 0.3 |longest path - qlen|)
    (poa_call::est_width) -- exceeds 1 000 columns, the width up to which a launch is k_poa_dp_t6's: with one of these in the
    batch VGA_POA_KERNEL=t7 reaches k_poa_dp_t7 instead."""
    rng = random.Random(seed)
    nodes, edges, arms = fan_graph(rng, [3200, 12, 12, 12, 12, 12])
    nodes[0] = _seq(rng, 1100)
    return [Case(f"wide-p{pos}-{kind}", "wide", (nodes, edges, fan_query(rng, nodes, arms, pos, kind))) for pos in (4, 5) for kind in ("clean", "del2", "del35")]


def fan_limit_problem(n, seed=7):
    """one fan of n equal arms, the last arm followed (the in-degree limit of the POA kernels is 255)"""
    rng = random.Random(seed + n)
    nodes, edges, arms = fan_graph(rng, [8] * n, join_len=40)
    return nodes, edges, fan_query(rng, nodes, arms, n - 1, "clean")


# ---------------------------------------------------------------- reach
def chain_graph(rng, n, skips, far_first=True, lo=1, hi=9):
    """a chain of n nodes of unequal length (so that the rows of the ring differ in width) with skip edges (a, b).  Edges are
    listed by destination; a node's skip edges come before its chain edge (far_first) or after it."""
    nodes = [_seq(rng, rng.randint(lo, hi)) for _ in range(n)]
    # a skip edge is only told from the chain by what follows it: keep the first base after the skip apart from the chain's
    for a, b in skips:
        if nodes[b][0] == nodes[a + 1][0]:
            nodes[b] = _other(rng, nodes[a + 1][0]) + nodes[b][1:]
    edges = []
    for v in range(1, n):
        far = sorted(a for a, b in skips if b == v)
        edges += [(a, v) for a in far] + [(v - 1, v)] if far_first else [(v - 1, v)] + [(a, v) for a in far]
    return nodes, edges


def chain_query(rng, nodes, taken, err=0.0):
    """walk the chain from node 0 to the last node, leaving it along every skip edge (a, b) of `taken`"""
    nxt = dict(taken)
    q, v = [], 0
    while v < len(nodes):
        q.append(nodes[v])
        v = nxt.get(v, v + 1)
    q = "".join(q)
    return "".join(c if rng.random() >= err else _other(rng, c) for c in q)


def reach_cases(seed=77):
    out = []
    for r in (31, 32, 33, 64, 200):
        for far_first in (True, False):
            rng = random.Random(seed * 1000 + r * 2 + far_first)
            nodes, edges = chain_graph(rng, r + 14, [(6, 6 + r)], far_first)
            tag = f"reach{r}-{'farfirst' if far_first else 'chainfirst'}"
            out.append(Case(tag + "-skip", "reach", (nodes, edges, chain_query(rng, nodes, [(6, 6 + r)]))))
            out.append(Case(tag + "-walk", "reach", (nodes, edges, chain_query(rng, nodes, []))))
            out.append(Case(tag + "-skip-noisy", "reach", (nodes, edges, chain_query(rng, nodes, [(6, 6 + r)], 0.03))))
    # several far-reaching nodes alive at once (their kept rows overlap), next to edges at and just under the ring's span
    rng = random.Random(seed + 1)
    skips = [(3, 40), (5, 38), (8, 75), (9, 41), (12, 44), (20, 90), (41, 74), (44, 76)]
    nodes, edges = chain_graph(rng, 100, skips)
    for name, taken in (("walk", []), ("a", [(3, 40), (41, 74)]), ("b", [(5, 38), (44, 76)]), ("c", [(8, 75)]), ("d", [(9, 41)]), ("e", [(12, 44), (44, 76)]),
                        ("f", [(20, 90)])):
        out.append(Case(f"reach-many-alive-{name}", "reach", (nodes, edges, chain_query(rng, nodes, taken, 0.02))))
    # a row that is read after the ring (33 slots) has wrapped a dozen times
    rng = random.Random(seed + 2)
    nodes, edges = chain_graph(rng, 440, [(4, 424), (10, 43)], lo=1, hi=5)
    out.append(Case("reach420-skip", "reach", (nodes, edges, chain_query(rng, nodes, [(4, 424)]))))
    out.append(Case("reach420-walk", "reach", (nodes, edges, chain_query(rng, nodes, [(10, 43)], 0.02))))
    # a far-reaching edge that lands on a node of in-degree 6: first and last of its predecessor list
    for far_first in (True, False):
        rng = random.Random(seed + 3 + far_first)
        v = 60
        skips = [(v - 45, v), (v - 5, v), (v - 4, v), (v - 3, v), (v - 2, v)]
        nodes, edges = chain_graph(rng, 75, skips, far_first, lo=2, hi=9)
        tag = f"reach45-indeg6-{'farfirst' if far_first else 'chainfirst'}"
        for a, _ in skips:
            out.append(Case(f"{tag}-from{a}", "reach", (nodes, edges, chain_query(rng, nodes, [(a, v)]))))
        out.append(Case(f"{tag}-walk", "reach", (nodes, edges, chain_query(rng, nodes, [], 0.02))))
        # the far edge taken and the first 35 bases after it missing from the read: a long deletion over a far predecessor
        q = chain_query(rng, nodes, [(v - 45, v)])
        cut = sum(len(nodes[x]) for x in range(v - 44))
        out.append(Case(f"{tag}-far-del35", "reach", (nodes, edges, q[:cut] + q[cut + 35:])))
        out.append(Case(f"{tag}-far-del2", "reach", (nodes, edges, q[:cut] + q[cut + 2:])))
    return out


# ---------------------------------------------------------------- sources and sinks
def source_sink_graph(rng, n_src, n_snk):
    """n_src source arms of different lengths -> one middle node -> n_snk sink arms of different lengths"""
    src_len = [(5, 60, 12, 33, 2, 90, 21, 8)[i] for i in range(n_src)]
    snk_len = [(70, 9, 25, 3, 48, 14, 100, 6)[i] for i in range(n_snk)]
    nodes = [_seq(rng, x) for x in src_len] + [_seq(rng, 50)] + [_seq(rng, x) for x in snk_len]
    mid = n_src
    edges = [(i, mid) for i in range(n_src)] + [(mid, mid + 1 + k) for k in range(n_snk)]
    return nodes, edges


def source_sink_cases(seed=5):
    out = []
    for n_src, n_snk in ((1, 1), (2, 3), (3, 2), (3, 3), (5, 1), (1, 8), (8, 8)):
        rng = random.Random(seed * 100 + n_src * 10 + n_snk)
        nodes, edges = source_sink_graph(rng, n_src, n_snk)
        mid = n_src
        for s in sorted({0, n_src // 2, n_src - 1}):
            for k in sorted({0, n_snk // 2, n_snk - 1, min(1, n_snk - 1)}):
                q = nodes[s] + nodes[mid] + nodes[mid + 1 + k]
                q = "".join(c if rng.random() >= 0.02 else _other(rng, c) for c in q)
                out.append(Case(f"src{n_src}-snk{n_snk}-s{s}-k{k}", "srcsink", (nodes, edges, q)))
    return out


# ---------------------------------------------------------------- random DAGs
def rand_dag_problem(rng, n_nodes, max_len, max_in=12, max_reach=80, qlen_scale=1.0):
    """`_rand_problem` of tests/test_gpu_parity.py with in-degree up to max_in and edges that reach up to max_reach nodes; the
    query is a random source-to-sink walk with the same mutation rates"""
    nodes = [_seq(rng, rng.randint(1, max_len)) for _ in range(n_nodes)]
    edges = []
    for v in range(1, n_nodes):
        srcs = {v - 1} if rng.random() < 0.8 else set()
        extra = rng.randint(0, max_in - 1) if rng.random() < 0.3 else rng.randint(0, 2)
        for _ in range(extra):
            srcs.add(rng.randint(max(0, v - max_reach), v - 1))
        srcs = sorted(srcs)
        if rng.random() < 0.5:
            rng.shuffle(srcs)
        edges += [(s, v) for s in srcs]
    out = {}
    for s, d in edges:
        out.setdefault(s, []).append(d)
    starts = [v for v in range(n_nodes) if v == 0 or all(d != v for _, d in edges)]
    path, v = [], rng.choice(starts)
    while True:
        path.append(v)
        if v not in out:
            break
        v = rng.choice(out[v])
    q = "".join(nodes[v] for v in path)
    q = q[: max(1, int(len(q) * qlen_scale))]
    ql = list(q)
    for i in range(len(ql)):
        x = rng.random()
        if x < 0.05:
            ql[i] = rng.choice("ACGT")
        elif x < 0.08:
            ql[i] = ql[i] + _seq(rng, rng.randint(1, 4))
        elif x < 0.11:
            ql[i] = ""
    return nodes, edges, "".join(ql) or "A"


def rand_dag_cases(seed=99, n=40):
    rng = random.Random(seed)
    return [Case(f"dag{i}", "dag", rand_dag_problem(rng, rng.randint(10, 140), rng.choice((3, 6, 12)))) for i in range(n)]


# ---------------------------------------------------------------- the fixed set, and what an oracle result went through
_fixed = None


def fixed_set():
    """the problems the GPU tests run, in a fixed order (built once)"""
    global _fixed
    if _fixed is None:
        _fixed = fan_cases() + reach_cases() + source_sink_cases() + rand_dag_cases()
    return _fixed


def pred_lists(n_nodes, edges):
    preds = [[] for _ in range(n_nodes)]
    for s, d in edges:
        preds[d].append(s)
    return preds


def node_steps(ref):
    """(cigar operation, node, length of the run of that operation it is part of) of every graph base of an oracle result, in
    path order"""
    ops, num = [], ""
    for c in ref.cigar:
        if c.isdigit():
            num += c
        else:
            ops += [(c, int(num))] * int(num)
            num = ""
    steps = [(op, run) for op, run in ops if op != "I"]
    assert len(steps) == len(ref.graph_nodes)
    return [(op, v, run) for (op, run), v in zip(steps, ref.graph_nodes)]


def deletion_piece(k, pen=DEFAULT_PEN):
    """which piece of the convex gap cost min(o1 + k e1, o2 + k e2) a deletion of k bases is charged by: "short", "long" or
    "tie" (under the default penalties 4 + 2k = 24 + k at k = 20)"""
    a, b = pen[2] + k * pen[3], pen[4] + k * pen[5]
    return "short" if a < b else "long" if a > b else "tie"


def classify(nodes, edges, ref, pen=DEFAULT_PEN):
    """For every node of in-degree > 1 the aligned path of the oracle result `ref` enters: (node, in-degree, position of the
    node it came from in the predecessor list, first operation on the node), the operation one of "match" (match or
    mismatch), "short", "long", "tie" (a deletion, by the piece of the gap cost its whole run is charged by)."""
    preds = pred_lists(len(nodes), edges)
    out, prev = [], None
    for op, v, run in node_steps(ref):
        if prev is not None and v != prev and len(preds[v]) > 1:
            out.append((v, len(preds[v]), preds[v].index(prev), "match" if op == "M" else deletion_piece(run, pen)))
        prev = v
    return out


def far_nodes_on_path(nodes, edges, ref):
    """(node, reach, whether the path left it along its farthest edge) for every node on the aligned path whose value row is
    read more than one node ahead; reach is the largest dst - src over its out-edges"""
    reach = [0] * len(nodes)
    for s, d in edges:
        reach[s] = max(reach[s], d - s)
    path = [v for i, (_, v, _) in enumerate(node_steps(ref)) if i == 0 or v != ref.graph_nodes[i - 1]]
    return [(a, reach[a], b - a == reach[a]) for a, b in zip(path, path[1:]) if reach[a] > 1]


# ---------------------------------------------------------------- a whole graph for vga_align_batch
AlignGraph = namedtuple("AlignGraph", "nodes edges bubbles far_edge reads")
Read = namedtuple("Read", "name seq walk")


def align_graph(seed=3, wide=40, n_skipped=40):
    """A few kbp of random sequence cut into nodes (ids from 1, in topological order), with a bubble of `wide` alleles, one of
    9 alleles and an edge that skips n_skipped nodes -- in a read's subgraph that edge reaches n_skipped + 1 nodes.  Reads are
    walks through chosen alleles with about 2 % errors.  bubbles: [(allele ids, join id)], far_edge: (src id, dst id)."""
    rng = random.Random(seed)
    nodes, edges = [], []

    def add(seq, preds):
        nodes.append((len(nodes) + 1, seq))
        edges.extend((p, len(nodes)) for p in preds)
        return len(nodes)

    def backbone(last, total):
        while total > 0:
            n = min(total, rng.randint(20, 60))
            last = add(_seq(rng, n), [last] if last else [])
            total -= n
        return last

    def bubble(last, n, lo, hi):
        alleles = [add(_seq(rng, rng.randint(lo, hi)), [last]) for _ in range(n)]
        return alleles, add(_seq(rng, 40), alleles)

    last = backbone(0, 400)
    wide_alleles, last = bubble(last, wide, 15, 30)
    last = backbone(last, 400)
    nine_alleles, last = bubble(last, 9, 18, 24)
    last = backbone(last, 300)
    skip_src = last
    for _ in range(n_skipped):
        last = add(_seq(rng, rng.randint(4, 12)), [last])
    skip_dst = add(_seq(rng, 40), [last, skip_src])
    last = backbone(skip_dst, 500)
    seq_of = dict(nodes)
    succ = {}
    for s, d in edges:
        succ.setdefault(s, []).append(d)
    reads = []
    picks = [(a, b, far) for a in (0, 3, 4, 5, wide // 2, wide - 1) for b, far in ((0, False), (4, True), (8, a % 2 == 0))]
    for a, b, far in picks:
        walk, v = [], 1
        while True:
            walk.append(v)
            if v not in succ:
                break
            nx = succ[v]
            v = nx[a % len(nx)] if nx[0] in wide_alleles else nx[b] if nx[0] in nine_alleles else skip_dst if (v == skip_src and far) else nx[0]
        s = "".join(seq_of[v] for v in walk)
        s = s[rng.randint(0, 150):len(s) - rng.randint(0, 150)]
        out = []
        for c in s:
            x = rng.random()
            out.append(_other(rng, c) if x < 0.01 else c + _seq(rng, 1) if x < 0.015 else "" if x < 0.02 else c)
        reads.append(Read(f"w{a}-n{b}-{'far' if far else 'chain'}", "".join(out), walk))
    return AlignGraph(nodes, edges, [(wide_alleles, wide_alleles[-1] + 1), (nine_alleles, nine_alleles[-1] + 1)], (skip_src, skip_dst), reads)
