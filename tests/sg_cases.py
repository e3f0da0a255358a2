"""Seeded reads that plant k_sg_mark / k_sg_emit (csrc/vga_subgraph.hip) on their fixed geometry: the 16 node ids of a bitmap
word, the 64 words of a pass of section A, the 64 nodes of a group of section D, the strict budget comparison and the re-queueing
of the extension walk, its 64-lane stride over the frontier, reverse handles, the 4-byte rounding of a problem's sequence bytes
-- what reads simulated from DRB1-3123 and the merged HLA graph leave to chance.

One graph of about 2 200 nodes with topological ids holds every family, so that one batch can mix them all (its components, in
id order: `build_graph`).  A read is cut from a path; a head or tail of bases that match nothing gives the walk a budget.  A case
is `(name, family, read)`.

The file has three further parts, all plain Python over what the oracle returns:
  * `reference` -- everything the kernels write for a problem (handles, first rows, predecessor list, sinks, the four words of
    every table entry, `remain` under both rules, longest, life, far-edge bits, wlo / whi, the sequence bytes), from the oracle's
    `subgraph_for_chain` alone: `range_handles`, `nodes`, `edges`;
  * `extension` -- an independent restatement of extend_range_chain_2 as a best-budget search per direction, which
    tests/test_sg_cases_cpu.py holds to the oracle's `range_handles` on every case;
  * `CELLS` -- per family, the predicates over `Facts` (the sg_desc values, the oracle's subgraph, the restated walk) that say which
    branch of the kernels a case reaches; tests/test_sg_cases_cpu.py fails on a cell that no case reaches.
tests/test_sg_cases_gpu.py holds the kernels' tables (VGA_SG_DUMP) to `reference`, field by field."""
import bisect
import heapq
import random
from collections import namedtuple

from poa_topologies import RING_SPAN  # = SG_RING_SPAN (tests/test_poa_topology_cpu.py guards it against the sources)

K = 11
WORD_IDS = 16    # node ids per bitmap word (32 packed handles)
PASS_WORDS = 64  # words per pass of section A of k_sg_emit
GROUP = 64       # nodes per group of section D
LINE = 16        # bases of a node of the lines

Read = namedtuple("Read", "name seq head tail")  # head / tail: bases in front of / behind the part cut from the path
Case = namedtuple("Case", "name family read")
GraphSpec = namedtuple("GraphSpec", "nodes edges")  # nodes: [sequence], id = index + 1; edges: [(left handle, right handle)], in insertion order


def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def pack(node_id, rev=False):
    return node_id * 2 + (1 if rev else 0)


# ---------------------------------------------------------------------------------------------------------------- the graph
class _Builder:
    def __init__(self, rng):
        self.rng, self.nodes, self.edges = rng, [], []

    def node(self, n, alphabet="ACGT", seq=None):
        self.nodes.append(seq if seq is not None else _seq(self.rng, n, alphabet))
        return len(self.nodes)

    def edge(self, a, b, arev=False, brev=False):
        self.edges.append((pack(a, arev), pack(b, brev)))

    def line(self, n, length=LINE):
        ids = [self.node(length) for _ in range(n)]
        for a, b in zip(ids, ids[1:]):
            self.edge(a, b)
        return ids


G_LINE = 140                 # the line of the word and group families: ids 1 .. 140
G_DECOYS = (50, 110)         # ... two of them without an edge (the line passes them by): sources and sinks of their own inside a range
G_SKIP_FIRST = ((2, 130), (67, 130))  # skip edges that come BEFORE the line edge in their source's edge list
G_SKIP_LAST = ((66, 130),)            # ... and one that comes after it
FANS = (65, 70, 130)
UNEQUAL_ARMS = (3, 2, 1, 2, 3)
CHAIN_END = 2200             # the chain of short nodes runs to about this id; three line nodes end the graph


def build_graph(seed=9100):
    """The graph of every family, as (GraphSpec, marks); marks names the ids the reads are cut from.  In id order:
      g      a line of 140 nodes of 16 bases with two unconnected decoys and three skip edges into node 130 (word, group);
      head   six nodes of 12 bases that lead, over a jump of some 620 ids, into the chain: a read from here to the chain's end
             spans 128 and 129 bitmap words, with every component in between inside its range (pass);
      dia    a diamond of one 6-base arm and three 1-base arms up- and downstream of a four-node line, a 5-base merge node and a
             4-base node behind it (budget);
      hub    a 3-base node behind a 5-base node, up- and downstream of a three-node line (budget);
      fan*   fans of 65, 70 and 130 one-base arms and one of five arms of 1 to 3 bases, each up- and downstream of a three-node
             line, a 2-base hub and a 4-base node behind it (frontier);
      strand a three-node line entered from the reverse strand of a node and left into the reverse strand of another, each with
             a letter outside ACGTU, beside plain forward neighbours (strand);
      chain  about 1 450 nodes of 1 to 4 bases with SNP and deletion bubbles, dead ends and unconnected decoys sprinkled in
             (pass, gap, N % 4), then three line nodes, the last of which is the graph's last id (word);
      far    edges 140 -> a chain node 128 words up and 20 -> the chain's last but one node: the neighbour a walk reaches lies more
             than two passes away (gap)."""
    rng = random.Random(seed)
    b = _Builder(rng)
    m = {}
    # g: the line edge of a node with a skip edge is added around it, in the order the first-edge rule is to see
    g = [b.node(3 if i + 1 == G_DECOYS[0] else 5 if i + 1 == G_DECOYS[1] else LINE) for i in range(G_LINE)]
    on_line = [v for v in g if v not in G_DECOYS]
    nxt = dict(zip(on_line, on_line[1:]))
    for v in on_line[:-1]:
        for s, d in G_SKIP_FIRST:
            if s == v:
                b.edge(s, d)
        b.edge(v, nxt[v])
        for s, d in G_SKIP_LAST:
            if s == v:
                b.edge(s, d)
    m["g"] = g
    m["head"] = b.line(6, 12)
    # dia
    z, mg, a6, c1, c2, c3 = b.node(4), b.node(5), b.node(6), b.node(1), b.node(1), b.node(1)
    ln = b.line(4)
    for s, d in ((z, mg), (mg, a6), (mg, c1), (c1, c2), (c2, c3), (a6, ln[0]), (c3, ln[0])):
        b.edge(s, d)
    a6d, d1, d2, d3, mgd, zd = b.node(6), b.node(1), b.node(1), b.node(1), b.node(5), b.node(4)
    for s, d in ((ln[-1], a6d), (ln[-1], d1), (d1, d2), (d2, d3), (a6d, mgd), (d3, mgd), (mgd, zd)):
        b.edge(s, d)
    m["dia"] = ln
    # hub
    y, x = b.node(3), b.node(5)
    ln = b.line(3)
    xd, yd = b.node(5), b.node(3)
    for s, d in ((y, x), (x, ln[0]), (ln[-1], xd), (xd, yd)):
        b.edge(s, d)
    m["hub"] = ln
    # fans: the arms take three letters, so that a head or tail can start with the fourth and extend no match into an arm
    for tag, arms in [("fan%d" % n, (1,) * n) for n in FANS] + [("fanu", UNEQUAL_ARMS)]:
        zu, hu = b.node(4), b.node(2)
        b.edge(zu, hu)
        up = [b.node(n, "ACG") for n in arms]
        ln = b.line(3)
        for a in up:
            b.edge(hu, a)
            b.edge(a, ln[0])
        down = [b.node(n, "ACG") for n in arms]
        hd, zd = b.node(2), b.node(4)
        for a in down:
            b.edge(ln[-1], a)
            b.edge(a, hd)
        b.edge(hd, zd)
        m[tag] = ln
    # strand
    p, r = b.node(6), b.node(8, seq="ACNGTUAC")
    ln = b.line(3)
    t, u = b.node(8, seq="GTUACNCA"), b.node(6)
    b.edge(p, ln[0])
    b.edge(r, ln[0], arev=True)        # r- -> first+ : the upstream walk finds the odd handle of r
    b.edge(ln[-1], t, brev=True)       # last+ -> t-
    b.edge(ln[-1], u)
    m["strand"] = ln
    # chain: `path` is the walk the reads are cut from
    b.edge(m["head"][-1], len(b.nodes) + 1)
    path, prev, since = list(m["head"]), None, 0
    while len(b.nodes) < CHAIN_END:
        v = b.node(rng.randint(1, 4))
        if prev is not None:
            b.edge(prev, v)
        path.append(v)
        prev, since = v, since + 1
        if since < 12:
            continue
        since = 0
        kind = rng.choice(("snp", "del", "tip", "decoy"))
        if kind == "snp":
            a1, a2, j = b.node(1), b.node(1), b.node(rng.randint(1, 4))
            for s, d in ((prev, a1), (prev, a2), (a1, j), (a2, j)):
                b.edge(s, d)
            path += [rng.choice((a1, a2)), j]
            prev = j
        elif kind == "del":
            dn, j = b.node(rng.randint(1, 4)), b.node(rng.randint(1, 4))
            for s, d in ((prev, dn), (prev, j), (dn, j)):
                b.edge(s, d)
            path += ([dn] if rng.random() < 0.5 else []) + [j]
            prev = j
        elif kind == "tip":
            b.edge(prev, b.node(rng.randint(1, 4)))
        else:
            b.node(rng.randint(1, 4))
    tail = b.line(3)
    b.edge(prev, tail[0])
    path += tail
    m["path"], m["tail"] = path, tail
    # far
    chain = [v for v in path if v not in m["head"] and v not in tail]
    # (in the second half of its word: the few nodes that the walk reaches in front of it stay in that word)
    m["far_up"] = next(v for v in chain if v // WORD_IDS >= G_LINE // WORD_IDS + 2 * PASS_WORDS and v % WORD_IDS >= 10)
    m["far_down"] = chain[-2]
    b.edge(G_LINE, m["far_up"])
    b.edge(20, m["far_down"])
    return GraphSpec(b.nodes, b.edges), m


def make_graph(oracle, spec):
    g = oracle.Graph()
    for i, s in enumerate(spec.nodes):
        g.create_handle(s, i + 1)
    for a, c in spec.edges:
        g.create_edge(a, c)
    return g


# ---------------------------------------------------------------------------------------------------------------- the reads
def _neighbour_bases(spec, v, before):
    """the bases that stand right in front of (behind) node v on some forward walk"""
    out = set()
    for a, c in spec.edges:
        if before and c == pack(v) and not a & 1:
            out.add(spec.nodes[(a >> 1) - 1][-1])
        elif not before and a == pack(v) and not c & 1:
            out.add(spec.nodes[(c >> 1) - 1][0])
    return out


def _junk(rng, n, avoid, at_end):
    """n random bases whose base next to the part cut from the path is none of `avoid`: the match cannot grow into them"""
    if n == 0:
        return ""
    free = [c for c in "ACGT" if c not in avoid]
    assert free, "every base stands next to the read: no head or tail can be told from the graph"
    s = _seq(rng, n - 1)
    return s + rng.choice(free) if at_end else rng.choice(free) + s


def cut(spec, rng, name, ids, head=0, tail=0, skip=0, drop=0):
    """the read of the walk `ids`, without the first `skip` bases of its first node and the last `drop` of its last one, between
    `head` and `tail` bases of junk"""
    body = "".join(spec.nodes[v - 1] for v in ids)
    first, last = spec.nodes[ids[0] - 1], spec.nodes[ids[-1] - 1]
    front = {first[skip - 1]} if skip else _neighbour_bases(spec, ids[0], True)
    back = {last[len(last) - drop]} if drop else _neighbour_bases(spec, ids[-1], False)
    seq = _junk(rng, head, front, True) + body[skip:len(body) - drop] + _junk(rng, tail, back, False)
    return Read(name, seq, head, tail)


def _g_walk(a, c):
    return [v for v in range(a, c + 1) if v not in G_DECOYS]


def _path_between(m, a, c):
    p = m["path"]
    return p[p.index(a):p.index(c) + 1]


def _first_in_word(m, w, lo=0):
    return next(v for v in m["path"] if v // WORD_IDS == w and v >= lo)


def _last_in_word(m, w):
    return [v for v in m["path"] if v // WORD_IDS == w][-1]


WORD_RANGES = ((1, 48), (16, 30), (17, 31), (15, 32), (17, 30), (20, 20))
PASS_SPANS = (63, 64, 65, 128, 129)
PASS_WLO = 48  # the first word of the 63- to 65-word reads
GROUP_RANGES = ((5, 5), (5, 6), (2, 64), (2, 65), (2, 66), (2, 128), (2, 129), (2, 130))
FAN_BUDGETS = {65: (1, 4), 70: (1, 2, 3, 4), 130: (1, 4)}
N4_NODES = 40  # path nodes of a read of the N % 4 family

_built = None


def all_cases(seed=9100):
    """(GraphSpec, marks, [Case]) -- built once"""
    global _built
    if _built is not None:
        return _built
    spec, m = build_graph(seed)
    rng = random.Random(seed + 1)
    out = []

    def add(family, name, ids, **kw):
        out.append(Case(name, family, cut(spec, rng, name, ids, **kw)))

    for a, c in WORD_RANGES:
        add("word", "word-%d-%d" % (a, c), _g_walk(a, c))
    add("word", "word-16-31-walks", _g_walk(16, 31), head=3, tail=3)
    add("word", "word-last-id", m["tail"])
    for w in PASS_SPANS:
        wlo = m["head"][0] // WORD_IDS if w > 100 else PASS_WLO
        add("pass", "pass-%dw" % w, _path_between(m, _first_in_word(m, wlo, m["head"][0]), _last_in_word(m, wlo + w - 1)))
    p = m["path"]
    add("gap", "gap-up", p[p.index(m["far_up"]):], head=2)
    add("gap", "gap-down", _g_walk(18, 20), tail=2)
    for a, c in GROUP_RANGES:
        add("group", "group-n%d" % (c - a + 1), _g_walk(a, c))
    add("budget", "budget-prefix0", m["hub"], head=3, skip=3)
    add("budget", "budget-prefix1", m["hub"], head=4, skip=3)
    add("budget", "budget-suffix0", m["hub"], tail=3, drop=3)
    add("budget", "budget-suffix1", m["hub"], tail=4, drop=3)
    add("budget", "budget-hub-5", m["hub"], head=5, tail=5)
    add("budget", "budget-hub-6", m["hub"], head=6, tail=6)
    add("budget", "budget-diamond", m["dia"], head=10, tail=10)
    for n in FANS:
        for bud in FAN_BUDGETS[n]:
            add("frontier", "fan%d-b%d" % (n, bud), m["fan%d" % n], head=bud, tail=bud)
    add("frontier", "fan-unequal-b4", m["fanu"], head=4, tail=4)
    add("strand", "strand-b3", m["strand"], head=3, tail=3)
    add("strand", "strand-b12", m["strand"], head=12, tail=12)
    # N % 4: two reads of every residue of the rows of their range (every id between the ends, whatever the path takes)
    chain = [v for v in p if v > m["strand"][-1] + 2 and v not in m["tail"]]
    taken = {0: 0, 1: 0, 2: 0, 3: 0}
    for i in range(60, len(chain) - N4_NODES, 37):
        ids = chain[i:i + N4_NODES]
        rows = sum(len(spec.nodes[v - 1]) for v in range(ids[0], ids[-1] + 1))
        if taken[rows % 4] < 2:
            taken[rows % 4] += 1
            add("n4", "n4-r%d-%d" % (rows % 4, taken[rows % 4]), ids)
    assert all(v == 2 for v in taken.values()), taken
    _built = (spec, m, out)
    return _built


FAMILIES = ("word", "pass", "gap", "group", "budget", "frontier", "strand", "n4")


def family(cases, name):
    return [c for c in cases if c.family == name]


# ------------------------------------------------------------------------------------------------------------ the reference
FIRST_EDGE, LONGEST_PATH = 1, 0
SUM_FIELDS = ("n_nodes", "N", "n_preds", "n_sinks", "wlo", "whi", "longest", "life", "flags")
LIST_FIELDS = ("handles", "first_row", "preds", "sinks", "table", "seq")  # table: (row, len, deg, sink, far, remain, pred) of the source and of every node


def reference(sub, rule):
    """What k_sg_mark / k_sg_emit write for the subgraph `sub` (oracle_py.SubgraphT) under remain rule `rule`, as a dict of the
    fields of SUM_FIELDS and LIST_FIELDS.  Uses sub.range_handles, sub.nodes and sub.edges only."""
    n = len(sub.nodes)
    lens = [len(s) for s in sub.nodes]
    first_row, rows = [], 0
    for ln in lens:
        first_row.append(rows + 1)
        rows += ln
    last_row = [f + ln - 1 for f, ln in zip(first_row, lens)]
    ins, outs = [[] for _ in range(n)], [[] for _ in range(n)]
    for s, d in sub.edges:  # (the oracle's order: by source, and for one source in the order of the index's edge list)
        ins[d].append(s)
        outs[s].append(d)
    # predecessor list: sources ascending; a node without one reads row 0, the virtual source
    preds, pred_word, degs = [], [], []
    for v in range(n):
        src = sorted(ins[v])
        degs.append(max(1, len(src)))
        pred_word.append(len(preds) if len(src) > 1 else (last_row[src[0]] if src else 0))
        preds += [last_row[s] for s in src] or [0]
    sinks = [last_row[v] for v in range(n) if not outs[v]]
    # remain of a node's last base and of its first (rf), last node first
    remain, rf = [0] * n, [0] * n
    for v in range(n - 1, -1, -1):
        if outs[v]:
            # the first-edge rule follows the first edge with this source in the oracle's edge order
            remain[v] = 1 + rf[outs[v][0]] if rule == FIRST_EDGE else max(1 + rf[d] for d in outs[v])
        rf[v] = remain[v] + lens[v] - 1
    sources = [v for v in range(n) if not ins[v]]
    longest = 1 + rf[sources[0]] if rule == FIRST_EDGE else max(1 + rf[v] for v in sources)
    reach = [max([d - v for d in outs[v]] or [0]) for v in range(n)]
    life = max([1] + [x for x in reach if x <= RING_SPAN])
    table = [(0, 1, 0, 0, 0, longest, 0)]
    for v in range(n):
        table.append((first_row[v], lens[v], degs[v], 0 if outs[v] else 1, 1 if reach[v] > RING_SPAN else 0, remain[v], pred_word[v]))
    hs = list(sub.range_handles)
    return dict(n_nodes=n, N=rows, n_preds=len(preds), n_sinks=len(sinks), wlo=hs[0] >> 5, whi=hs[-1] >> 5, longest=longest, life=life, flags=0,
                handles=hs, first_row=first_row, preds=preds, sinks=sinks, table=table, seq="".join(sub.nodes))


def parse_dump(text):
    """the records of a VGA_SG_DUMP file, in file (launch) order: dicts of `read`, `desc` and the fields of `reference`"""
    out, cur = [], None
    for ln in text.splitlines():
        f = ln.split()
        tag, v = f[0], f[1:]
        if tag == "P":
            cur = dict(problem=int(v[0]), read=int(v[2]), desc=tuple(int(x) for x in v[3:]), table=[])
            assert v[1] == "read" and len(cur["desc"]) == 7, ln
            out.append(cur)
        elif tag == "S":
            cur.update(zip(SUM_FIELDS, (int(x) for x in v)))
        elif tag == "T":
            assert int(v[0]) == len(cur["table"]), ln
            cur["table"].append(tuple(int(x) for x in v[1:]))
        elif tag in "HFLK":
            cur[{"H": "handles", "F": "first_row", "L": "preds", "K": "sinks"}[tag]] = [int(x) for x in v]
        elif tag == "Q":
            cur["seq"] = bytes.fromhex(v[0] if v else "").decode("latin-1")
        else:
            assert tag == "E", ln
    return out


def differences(got, want):
    """the fields of a dump record that differ from the reference, with the first differing position of a list"""
    out = []
    for k in SUM_FIELDS:
        if got.get(k) != want[k]:
            out.append((k, got.get(k), want[k]))
    for k in LIST_FIELDS:
        g, w = got.get(k), want[k]
        if g != w:
            at = next((i for i, (x, y) in enumerate(zip(g or [], w)) if x != y), min(len(g or []), len(w)))
            out.append((k, at, (g or [None])[at] if g and at < len(g) else None, w[at] if at < len(w) else None))
    return out


# ------------------------------------------------------------------------------------------------ the chain and its subgraph
DESC_FIELDS = ("pmin", "pmax", "q_first", "t_first", "q_last", "te_last", "qlen")


def desc_of(chain, qlen):
    """the sg_desc of a chain (align_plan_problem, csrc/vga_align_plan.hpp): `chain` is the oracle's list of anchors"""
    pos = [a.target_begin[1] for a in chain] + [a.target_end[1] - 1 for a in chain]
    return dict(pmin=min(pos), pmax=max(pos), q_first=chain[0].query_begin, t_first=chain[0].target_begin[1], q_last=chain[-1].query_begin,
                te_last=chain[-1].target_end[1], qlen=qlen)


class IndexView:
    """what the walk needs of an oracle index, read once: node starts, lengths and the neighbour lists of the forward handles"""

    def __init__(self, ix):
        ref = ix.node_ref()
        self.start = [r[0] for r in ref]  # start[id - 1] .. start[id]: the bases of node id
        self.n_nodes = len(ref) - 1
        edges = ix.edges()
        self.inc = [edges[ref[i][1]:ref[i][1] + ref[i][2]] for i in range(self.n_nodes)]
        self.out = [edges[ref[i][1] + ref[i][2]:ref[i + 1][1]] for i in range(self.n_nodes)]

    def node_at(self, pos):
        return bisect.bisect_right(self.start, pos)

    def length(self, h):
        return self.start[h >> 1] - self.start[(h >> 1) - 1]

    def neighbours(self, h, incoming):
        """a reverse handle takes the other list of its forward twin, every entry flipped"""
        lst = (self.inc if incoming != bool(h & 1) else self.out)[(h >> 1) - 1]
        return [x ^ (h & 1) for x in lst]


def budgets(view, desc, k=K):
    """(min_id, max_id, prefix_diff, suffix_diff): the range of find_range_chain and the two budgets of extend_range_chain_2"""
    lo, hi = view.node_at(desc["pmin"]), view.node_at(desc["pmax"])
    on_first = desc["t_first"] - view.start[lo - 1]
    prefix = desc["q_first"] - on_first if on_first < desc["q_first"] else 0
    suffix = desc["qlen"] - (desc["q_last"] + k)
    on_last = view.start[hi] - 1 - (desc["te_last"] - 1)
    suffix = 0 if on_last > suffix else suffix - on_last
    return lo, hi, prefix, suffix


def best_budgets(view, start, budget, incoming):
    """{handle: the largest budget it is reached with}, walking from `start`: a handle hands budget - length on, and only while
    its length is smaller than its budget (largest budget first, so that every handle is settled once)"""
    best, heap = {}, [(-budget, x) for x in view.neighbours(start, incoming)] if budget > 0 else []
    heapq.heapify(heap)
    while heap:
        left, h = heapq.heappop(heap)
        left = -left
        if h in best:
            continue
        best[h] = left
        if view.length(h) < left:
            for x in view.neighbours(h, incoming):
                if x not in best:
                    heapq.heappush(heap, (-(left - view.length(h)), x))
    return best


def extension(view, desc):
    """the handle set of a chain, restated: every forward handle of the range and what either walk reaches.  Returns
    (sorted handles, budgets upstream, budgets downstream)"""
    lo, hi, prefix, suffix = budgets(view, desc)
    up = best_budgets(view, pack(lo), prefix, True)
    down = best_budgets(view, pack(hi), suffix, False)
    return sorted(set(pack(v) for v in range(lo, hi + 1)) | set(up) | set(down)), up, down


def levels(view, start, budget, incoming):
    """{handle: [(level, budget)]}: every improvement of a handle's budget in a walk that advances one neighbour list per level
    (sg_extend's order), for the predicates on re-queueing"""
    seen, cur, level = {}, [], 1
    for x in view.neighbours(start, incoming) if budget > 0 else []:
        if not seen.get(x):
            seen[x] = [(level, budget)]
            cur.append(x)
    while cur:
        level += 1
        nxt = []
        for h in cur:
            left = seen[h][-1][1]
            if view.length(h) < left:
                for x in view.neighbours(h, incoming):
                    rem = left - view.length(h)
                    if x not in seen or seen[x][-1][1] < rem:
                        if x in seen and seen[x][-1][0] == level:
                            seen[x][-1] = (level, rem)
                        else:
                            seen.setdefault(x, []).append((level, rem))
                        if x not in nxt:
                            nxt.append(x)
        cur = nxt
    return seen


Facts = namedtuple("Facts", "case desc sub view spec lo hi prefix suffix up down ref")  # ref: {rule: reference}


def facts_of(oracle, ix, view, spec, case):
    """Runs the oracle on the case's read: its best chain, the subgraph of that chain, and everything the predicates look at"""
    res, cs, arr = oracle.chain_anchors(ix, case.read.seq, keep_raw=True)
    try:
        assert res.chains and not res.is_placeholder[0], case.name + ": no chain"
        sub, _ = oracle.subgraph_for_chain(ix, cs, 0, len(case.read.seq))
    finally:
        oracle.lib().og_chain_set_free(cs)
        if res.sorted_anchors:
            oracle.lib().og_free(arr)
    desc = desc_of(res.chains[0], len(case.read.seq))
    lo, hi, prefix, suffix = budgets(view, desc)
    _, up, down = extension(view, desc)
    return Facts(case, desc, sub, view, spec, lo, hi, prefix, suffix, up, down, {r: reference(sub, r) for r in (LONGEST_PATH, FIRST_EDGE)}), res


# ------------------------------------------------------------------------------------------------------------ the predicates
def _words(f):
    return f.sub.range_handles[0] >> 5, f.sub.range_handles[-1] >> 5


def _one_beside(f, below):
    """the walk added exactly one handle, in the word next to the range's first (last) word, and nothing further out"""
    w = pack(f.lo) >> 5 if below else pack(f.hi) >> 5
    extra = [h for h in f.sub.range_handles if (h >> 5 < w if below else h >> 5 > w)]
    return len(extra) == 1 and extra[0] >> 5 == (w - 1 if below else w + 1)


def _carries(f):
    """the running sums of section A behind its first pass: nodes, rows, predecessor entries and sink entries of the words
    wlo .. wlo + 63"""
    wlo, _ = _words(f)
    t = f.ref[FIRST_EDGE]["table"][1:]
    sel = [x for h, x in zip(f.sub.range_handles, t) if (h >> 5) - wlo < PASS_WORDS]
    return len(sel), sum(x[1] for x in sel), sum(x[2] for x in sel), sum(x[3] for x in sel)


def _pass_cell(span):
    def p(f):
        wlo, whi = _words(f)
        return wlo > 0 and whi - wlo + 1 == span
    return p


def _empty_pass(f):
    """a pass of section A (64 words from wlo on) without a member, with members behind it"""
    wlo, whi = _words(f)
    used = {(h >> 5) - wlo for h in f.sub.range_handles}
    return any(not any(w in used for w in range(p0, p0 + PASS_WORDS)) for p0 in range(PASS_WORDS, whi - wlo + 1 - PASS_WORDS, PASS_WORDS))


def _far_neighbour(f, incoming):
    got = f.up if incoming else f.down
    edge = pack(f.lo) >> 5 if incoming else pack(f.hi) >> 5
    return any(abs((h >> 5) - edge) > PASS_WORDS for h in got)


def _isolated_inside(f):
    n = len(f.sub.nodes)
    touched = {s for s, _ in f.sub.edges} | {d for _, d in f.sub.edges}
    return any(v not in touched for v in range(1, n - 1))


def _group_of(f, v):
    return (len(f.sub.nodes) - 1 - v) // GROUP  # groups are counted from the top rank down


def _edge(test):
    return lambda f: any(test(f, s, d) for s, d in f.sub.edges)


def _sources(f):
    n = len(f.sub.nodes)
    has_in = {d for _, d in f.sub.edges}
    return [v for v in range(n) if v not in has_in]


def _first_source_late(f):
    src = _sources(f)
    return len({_group_of(f, v) for v in src}) > 1 and _group_of(f, src[0]) > min(_group_of(f, v) for v in src)


def _first_out_edge_leaves(f):
    """a member whose first out-neighbour in the index's list is not a later member of the set, while a later entry is one"""
    members = set(f.sub.range_handles)
    for h in f.sub.range_handles:
        nb = [y in members and y > h for y in f.view.neighbours(h, False)]
        if len(nb) > 1 and not nb[0] and any(nb[1:]):
            return True
    return False


def rules_differ(f):
    a, b = f.ref[LONGEST_PATH], f.ref[FIRST_EDGE]
    return [x[5] for x in a["table"]] != [x[5] for x in b["table"]]


def _stops(f, incoming, slack):
    """a handle the walk reached with a budget of its length + slack: at 0 it is not expanded, at 1 it is, with 1 to hand on"""
    got = f.up if incoming else f.down
    hit = [h for h, left in got.items() if left == f.view.length(h) + slack]
    if slack == 0:
        return bool(hit)
    return any(any(got.get(x) == 1 for x in f.view.neighbours(h, incoming)) for h in hit)


def _requeued(f, incoming):
    """a handle whose budget improves at a later level, from one that does not let it expand to one that does: what lies behind
    it is reached by the larger budget only"""
    start, budget = (pack(f.lo), f.prefix) if incoming else (pack(f.hi), f.suffix)
    for h, steps in levels(f.view, start, budget, incoming).items():
        if len(steps) > 1 and steps[0][1] <= f.view.length(h) < steps[-1][1]:
            return True
    return False


def _fan(n, incoming):
    """the first level of the walk is n one-base arms -- more than the 64 lanes of a stride -- and all of them relax one hub"""
    def p(f):
        start, budget = (pack(f.lo), f.prefix) if incoming else (pack(f.hi), f.suffix)
        arms = f.view.neighbours(start, incoming) if budget > 0 else []
        if len(arms) != n or any(f.view.length(a) != 1 for a in arms):
            return False
        hubs = {x for a in arms for x in f.view.neighbours(a, incoming)}
        got = f.up if incoming else f.down
        return len(hubs) == 1 and budget >= 2 and hubs <= set(got)
    return p


def _whole_fan_only(incoming):
    """budget 1: the arms are taken, all of them, and nothing behind them"""
    def p(f):
        start, budget = (pack(f.lo), f.prefix) if incoming else (pack(f.hi), f.suffix)
        arms = f.view.neighbours(start, incoming)
        got = f.up if incoming else f.down
        return budget == 1 and len(arms) > PASS_WORDS and set(got) == set(arms)
    return p


def _shortest_arm_decides(f, incoming):
    """a hub behind arms of unequal length that is expanded with the budget the shortest arm hands on, and would not be with the
    next best one"""
    start, budget = (pack(f.lo), f.prefix) if incoming else (pack(f.hi), f.suffix)
    arms = f.view.neighbours(start, incoming) if budget > 0 else []
    got = f.up if incoming else f.down
    if len({f.view.length(a) for a in arms}) < 2:
        return False
    for hub in {x for a in arms for x in f.view.neighbours(a, incoming)}:
        handed = sorted({budget - f.view.length(a) for a in arms if f.view.length(a) < budget and hub in f.view.neighbours(a, incoming)})
        if len(handed) > 1 and got.get(hub) == handed[-1] and handed[-2] <= f.view.length(hub) < handed[-1]:
            return True
    return False


def _odd_with_foreign_letter(f, incoming):
    got = f.up if incoming else f.down
    return any(h & 1 and h in f.sub.range_handles and set(f.spec.nodes[(h >> 1) - 1]) - set("ACGTUacgtu") and "N" in f.sub.nodes[f.sub.range_handles.index(h)]
               for h in got)


def _n4(r):
    return lambda f: f.case.family == "n4" and f.ref[FIRST_EDGE]["N"] % 4 == r


# family -> [(cell, predicate, cases needed)]
CELLS = {
    "word": [("min_id %% 16 == %d" % r, (lambda r: lambda f: f.lo % WORD_IDS == r)(r), 1) for r in (0, 1, 15)]
    + [("max_id %% 16 == %d" % r, (lambda r: lambda f: f.hi % WORD_IDS == r)(r), 1) for r in (0, 14, 15)]
    + [("first and last handle in one word", lambda f: f.lo < f.hi and pack(f.lo) >> 5 == pack(f.hi) >> 5 and _words(f) == (pack(f.lo) >> 5,) * 2, 1),
       ("one-node range", lambda f: f.lo == f.hi, 1),
       ("node id 1 is a range end", lambda f: f.lo == 1, 1),
       ("the graph's last id is a range end", lambda f: f.hi == f.view.n_nodes, 1),
       ("walk adds one handle, in the word below wlo", lambda f: _one_beside(f, True), 1),
       ("walk adds one handle, in the word above whi", lambda f: _one_beside(f, False), 1)],
    "pass": [("span of %d words, wlo > 0" % w, _pass_cell(w), 1) for w in PASS_SPANS]
    + [("node lengths 1, 2, 3 and 4", lambda f: {1, 2, 3, 4} <= {len(s) for s in f.sub.nodes}, 1),
       ("four distinct non-zero sums carried into the second pass", lambda f: _words(f)[1] - _words(f)[0] >= PASS_WORDS and 0 < min(_carries(f))
        and len(set(_carries(f))) == 4, 1)],
    "gap": [("upstream neighbour more than 64 words from the range", lambda f: _far_neighbour(f, True), 1),
            ("downstream neighbour more than 64 words from the range", lambda f: _far_neighbour(f, False), 1),
            ("a whole pass of empty words, walk upstream", lambda f: _far_neighbour(f, True) and _empty_pass(f), 1),
            ("a whole pass of empty words, walk downstream", lambda f: _far_neighbour(f, False) and _empty_pass(f), 1),
            ("unconnected node inside the range", _isolated_inside, 1)],
    "group": [("n_nodes == %d" % n, (lambda n: lambda f: len(f.sub.nodes) == n)(n), 1) for n in (1, 2, 63, 64, 65, 127, 128, 129)]
    + [("edge of 63 ranks inside one group, from its top", _edge(lambda f, s, d: d - s == GROUP - 1 and (len(f.sub.nodes) - 1 - d) % GROUP == 0), 1),
       ("edge of 64 ranks into the next group", _edge(lambda f, s, d: d - s == GROUP), 1),
       ("edge that skips a whole group", _edge(lambda f, s, d: _group_of(f, s) - _group_of(f, d) >= 2), 1),
       ("successor is the top node of the group", _edge(lambda f, s, d: _group_of(f, s) == _group_of(f, d) and (len(f.sub.nodes) - 1 - d) % GROUP == 0), 1),
       ("successor is the first node above the group", _edge(lambda f, s, d: _group_of(f, s) == _group_of(f, d) + 1
                                                            and (len(f.sub.nodes) - 1 - d) % GROUP == GROUP - 1), 1),
       ("sources in several groups, the first one found in a later group", _first_source_late, 1),
       ("first out-edge in index order leaves the set", _first_out_edge_leaves, 1)],
    "budget": [("prefix_diff == 0 behind a head", lambda f: f.desc["q_first"] > 0 and f.prefix == 0, 1),
               ("prefix_diff == 1", lambda f: f.prefix == 1, 1),
               ("suffix_diff == 0 in front of a tail", lambda f: f.desc["q_last"] + K < f.desc["qlen"] and f.suffix == 0, 1),
               ("suffix_diff == 1", lambda f: f.suffix == 1, 1),
               ("upstream: length == budget, not expanded", lambda f: _stops(f, True, 0), 1),
               ("upstream: length == budget - 1, expanded", lambda f: _stops(f, True, 1), 1),
               ("downstream: length == budget, not expanded", lambda f: _stops(f, False, 0), 1),
               ("downstream: length == budget - 1, expanded", lambda f: _stops(f, False, 1), 1),
               ("upstream: merge node improved at a later level", lambda f: _requeued(f, True), 1),
               ("downstream: merge node improved at a later level", lambda f: _requeued(f, False), 1)],
    "frontier": [("%d arms %s, hub relaxed by all" % (n, "upstream" if inc else "downstream"), _fan(n, inc), 1) for n in FANS for inc in (True, False)]
    + [("whole fan at budget 1, upstream", _whole_fan_only(True), 1), ("whole fan at budget 1, downstream", _whole_fan_only(False), 1),
       ("shortest arm decides the hub, upstream", lambda f: _shortest_arm_decides(f, True), 1),
       ("shortest arm decides the hub, downstream", lambda f: _shortest_arm_decides(f, False), 1)],
    "strand": [("odd handle with a letter outside ACGTU, upstream", lambda f: _odd_with_foreign_letter(f, True), 1),
               ("odd handle with a letter outside ACGTU, downstream", lambda f: _odd_with_foreign_letter(f, False), 1)],
    "n4": [("N %% 4 == %d, twice in the batch" % r, _n4(r), 2) for r in range(4)],
}
# the cells whose cases must include one on which the two remain rules give a different `remain`
RULE_SENSITIVE = ("edge of 63 ranks inside one group, from its top", "edge of 64 ranks into the next group", "edge that skips a whole group",
                  "sources in several groups, the first one found in a later group", "first out-edge in index order leaves the set")


def table(facts, fam):
    """[(cell, needed, [case names that reach it], [... on which the remain rules differ])] of one family; a case of any family
    counts"""
    out = []
    for cell, pred, need in CELLS[fam]:
        hit = [f for f in facts if pred(f)]
        out.append((cell, need, [f.case.name for f in hit], [f.case.name for f in hit if rules_differ(f)]))
    return out
