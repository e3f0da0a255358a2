"""Planted cases for k_gaf_chain_len / k_gaf_chain_write (csrc/vga_gaf.hip, behind vga_chain_paths_text), and a plain reference of
the path column they write.  Simulated reads on the HLA graphs give node ids of at most five digits, offsets of at most four, and
whatever chain lengths the reads happen to have; here a synthetic graph puts every digit count of the four numbers of an anchor on
both sides of each power of ten, and the chains are laid out by hand: member counts around the 64-anchor rounds of the write pass,
text lengths mixed inside a round, chain counts around the launch grid, placeholders, reads without anchors.  Plain Python and
numpy: no GPU, no oracle.

A case is a vga_map_result built from arrays (`Case.result()` gives the ctypes object Context.chain_paths_text takes); only the
fields vga_chain_paths_text reads are filled.  `reference(case)` is the expected text per chain; tests/test_chain_text_cases_cpu.py
shows from that text alone that the cases hold the conditions they are there for, and pins the reference to the oracle's chains GAF."""
import ctypes as C
import functools
import random
import re

import numpy as np

# ---------------------------------------------------------------- the reference
ANCHOR_RE = re.compile(rb"\(>(\d+):(\d+),>(\d+):(\d+)\),")


def anchor_numbers(node_start, tb, te):
    """per anchor (first node, offset in it, last node, offset in it): the node of a position is 1 + the index of the last node
    start <= the position, taken for target_begin and for the inclusive end target_end - 1"""
    ns = np.asarray(node_start, dtype=np.int64)
    first, last = np.asarray(tb, dtype=np.int64), np.asarray(te, dtype=np.int64) - 1
    fn = np.searchsorted(ns, first, side="right")
    ln = np.searchsorted(ns, last, side="right")
    return fn, first - ns[fn - 1], ln, last - ns[ln - 1]


def anchor_texts(node_start, tb, te):
    fn, fo, ln, lo = anchor_numbers(node_start, tb, te)
    return [b"(>%d:%d,>%d:%d)," % q for q in zip(fn.tolist(), fo.tolist(), ln.tolist(), lo.tolist())]


def path_column(node_start, tb, te, members):
    """the path column of one chain: "(>N:off,>N:off)," for each of its anchors tb[i], te[i], i in members, in order"""
    m = list(members)
    return b"".join(anchor_texts(node_start, [tb[i] for i in m], [te[i] for i in m]))


# ---------------------------------------------------------------- a vga_map_result from arrays
class Case:
    """the fields of a vga_map_result that vga_chain_paths_text reads.  Chain c belongs to the read r with chain_off[r] <= c <
    chain_off[r + 1]; its members are anchor_off[r] + chain_anchor_idx[chain_anchor_off[c] .. chain_anchor_off[c + 1]), none for
    a placeholder."""

    def __init__(self, name, graph, anchor_off, tb, te, chain_off, placeholder, chain_anchor_off, chain_anchor_idx):
        self.name, self.graph = name, graph
        self.anchor_off = np.ascontiguousarray(anchor_off, dtype=np.uint64)
        self.target_begin = np.ascontiguousarray(tb, dtype=np.uint32)
        self.target_end = np.ascontiguousarray(te, dtype=np.uint32)
        self.chain_off = np.ascontiguousarray(chain_off, dtype=np.uint64)
        self.chain_placeholder = np.ascontiguousarray(placeholder, dtype=np.uint8)
        self.chain_anchor_off = np.ascontiguousarray(chain_anchor_off, dtype=np.uint64)
        self.chain_anchor_idx = np.ascontiguousarray(chain_anchor_idx, dtype=np.uint32)
        self.n_reads, self.n_anchors, self.n_chains = len(self.anchor_off) - 1, len(self.target_begin), len(self.chain_placeholder)
        assert len(self.chain_off) == self.n_reads + 1 and len(self.chain_anchor_off) == self.n_chains + 1
        assert int(self.anchor_off[-1]) == self.n_anchors and int(self.chain_off[-1]) == self.n_chains
        assert int(self.chain_anchor_off[-1]) == len(self.chain_anchor_idx)

    def __repr__(self):
        return self.name

    def members(self, c):
        """the anchors of chain c as indices into target_begin / target_end"""
        r = int(np.searchsorted(self.chain_off, c, side="right")) - 1
        if self.chain_placeholder[c]:
            return []
        s, e = int(self.chain_anchor_off[c]), int(self.chain_anchor_off[c + 1])
        return (int(self.anchor_off[r]) + self.chain_anchor_idx[s:e].astype(np.int64)).tolist()

    def result(self):
        """a MapResult (binding.py) over this case's arrays, with the `_ptr` Context.chain_paths_text passes on; the arrays
        stay alive on the returned object"""
        from helpers import pkg

        b = pkg().binding
        m = b.MapResult()
        m.n_reads, m.n_anchors, m.n_chains = self.n_reads, self.n_anchors, self.n_chains
        for name, ctype in (("anchor_off", C.c_uint64), ("target_begin", C.c_uint32), ("target_end", C.c_uint32), ("chain_off", C.c_uint64),
                            ("chain_placeholder", C.c_uint8), ("chain_anchor_off", C.c_uint64), ("chain_anchor_idx", C.c_uint32)):
            setattr(m, name, getattr(self, name).ctypes.data_as(C.POINTER(ctype)))
        m._keep = self
        m._ptr = C.pointer(m)
        return m


def build_case(name, graph, reads):
    """reads: [(anchors [(tb, te), ...], chains [None for a placeholder | [index into the read's anchors, ...], ...]), ...]"""
    anchor_off, chain_off, cao = [0], [0], [0]
    tb, te, ph, idx = [], [], [], []
    for anchors, chains in reads:
        tb += [a[0] for a in anchors]
        te += [a[1] for a in anchors]
        anchor_off.append(len(tb))
        for ch in chains:
            ph.append(1 if ch is None else 0)
            for i in ch or []:
                assert 0 <= i < len(anchors)
                idx.append(i)
            cao.append(len(idx))
        chain_off.append(len(ph))
    return Case(name, graph, anchor_off, tb, te, chain_off, ph, cao, idx)


def reference(case):
    """[bytes per chain]: the text vga_chain_paths_text owes for the case"""
    txt = anchor_texts(case.graph.node_start, case.target_begin, case.target_end)
    return [b"".join(txt[i] for i in case.members(c)) for c in range(case.n_chains)]


def describe_first_difference(case, got, want):
    """names the first chain whose text differs, the first anchor of it whose bytes differ, and that anchor's four numbers"""
    if len(got) != len(want):
        return "%s: %d chains on the GPU, %d expected" % (case.name, len(got), len(want))
    for c, (g, w) in enumerate(zip(got, want)):
        if g == w:
            continue
        mem = case.members(c)
        parts = anchor_texts(case.graph.node_start, case.target_begin[mem], case.target_end[mem])
        at = 0
        for j, t in enumerate(parts):
            if g[at:at + len(t)] != t:
                fn, fo, ln, lo = (int(x[0]) for x in anchor_numbers(case.graph.node_start, case.target_begin[mem[j]:mem[j] + 1],
                                                                     case.target_end[mem[j]:mem[j] + 1]))
                return ("%s: chain %d of %d (%d anchors, %d bytes on the GPU, %d expected) differs first at its anchor %d (anchor %d of the result, "
                        "text offset %d): first node %d offset %d, last node %d offset %d; expected %r, got %r"
                        % (case.name, c, len(want), len(mem), len(g), len(w), j, mem[j], at, fn, fo, ln, lo, t, g[at:at + len(t)]))
            at += len(t)
        return "%s: chain %d of %d is %d bytes on the GPU, %d expected, and equal up to there" % (case.name, c, len(want), len(g), len(w))
    return None


# ---------------------------------------------------------------- the synthetic graphs
class Graph:
    """a graph as vga_chain_paths_text sees it: the node starts.  upload() gives the context an index over it -- one repeated
    letter, no edges, k = 1 and the smallest valid k-mer half (one key, its forward record and the delimiter)."""

    def __init__(self, name, node_lengths):
        self.name = name
        self.node_start = np.concatenate(([0], np.cumsum(np.asarray(node_lengths, dtype=np.uint64)))).astype(np.uint64)
        self.n_nodes = len(self.node_start) - 1
        self.seq_length = int(self.node_start[-1])

    def pos(self, node_id, offset=0):
        assert 1 <= node_id <= self.n_nodes and 0 <= offset < self.node_length(node_id)
        return int(self.node_start[node_id - 1]) + offset

    def node_length(self, node_id):
        return int(self.node_start[node_id]) - int(self.node_start[node_id - 1])

    def upload(self, ctx):
        from helpers import pkg

        tab = np.zeros(2, dtype=pkg().binding.KMERPOS_DTYPE)
        tab[0] = (0, 1, 0, 0)
        tab[1] = (2 ** 64 - 1, 2 ** 64 - 1, 1, 1)
        zeros = np.zeros(self.n_nodes + 1, dtype=np.uint64)
        ctx.upload_index(1, b"A" * self.seq_length, self.node_start, zeros, zeros, np.zeros(0, dtype=np.uint64), b"A", [0], tab)


NODE1 = 100000001                                     # offsets of up to 9 digits
SMALL_NODES = (1, 2, 10, 11, 100, 1001, 10001, 1)     # nodes 2 to 9
LAST_NODE = 1000001                                   # ids of up to 7 digits: one-base nodes from 10 up to here
OFFSET_EDGES = tuple(10 ** d for d in range(1, 9))    # 9/10 .. 99 999 999/100 000 000
ID_EDGES = tuple(10 ** d for d in range(1, 7))        # 9/10 .. 999 999/1 000 000
MEMBER_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 200)
CHAIN_COUNTS = (1, 8191, 8192, 8193, 40000)           # 8192 = 32 x 256 CUs, the launch grid; 40 000 is beyond it on any CU count
SHORTEST, LONGEST = 12, 28                            # "(>1:0,>1:0)," and "(>1:100000000,>1:100000000),": a node whose id has
                                                      # more than one digit has offsets of at most five, so 28 is the graph's limit


@functools.lru_cache(maxsize=None)
def digits_graph():
    return Graph("digits", (NODE1,) + SMALL_NODES + (1,) * (LAST_NODE - 1 - len(SMALL_NODES)))


def _digits(v):
    return len("%d" % v)


def _anchor_of_length(g, rng, length):
    """an anchor inside node 1 whose text has `length` bytes: 8 + 1 + digits(fo) + 1 + digits(lo)"""
    d = length - 10
    lo_d = rng.randint(max(1, d - 9), min(9, d - 1))
    fo_d = d - lo_d
    if fo_d > lo_d:
        fo_d, lo_d = lo_d, fo_d
    pick = lambda n: rng.randint(0 if n == 1 else 10 ** (n - 1), min(10 ** n - 1, NODE1 - 1))
    fo, lo = pick(fo_d), pick(lo_d)
    if fo > lo:
        fo, lo = lo, fo
    return (fo, lo + 1)


def _random_position(g, rng):
    kind = rng.randrange(3)
    if kind == 0:
        return _anchor_of_length(g, rng, rng.randint(SHORTEST, LONGEST))[0]
    if kind == 1:
        node = rng.randint(2, 9)
        return g.pos(node, rng.randrange(g.node_length(node)))
    d = rng.randint(2, 7)
    return g.pos(rng.randint(10 ** (d - 1), min(10 ** d - 1, LAST_NODE)))


def _random_anchor(g, rng):
    """two positions of any kind, in order: the anchor may span any number of nodes"""
    a, b = sorted((_random_position(g, rng), _random_position(g, rng)))
    return (a, b + 1)


def edge_case(seed=5100):
    """each of the four numbers of an anchor on both sides of every power of ten it can cross, the other three at random; then the
    edge positions: tb = 0, te = seq_length, the last base of a node to the first of the next, an inclusive end on the last base
    of a node, a one-base anchor, node 1 to the last node.  One read, one chain per anchor and one chain over all of them."""
    g, rng = digits_graph(), random.Random(seed)
    anchors = []
    for e in OFFSET_EDGES:
        for v in (e - 1, e):
            anchors.append((v, max(v, _random_position(g, rng)) + 1))                       # fo = v
            anchors.append((rng.randint(0, v), v + 1))                                      # lo = v
    for e in ID_EDGES:
        for v in (e - 1, e):
            p = g.pos(v)
            anchors.append((p, max(p, _random_position(g, rng)) + 1))                       # fn = v
            anchors.append((min(p, _random_position(g, rng)), p + g.node_length(v)))        # ln = v (on its last base)
    L = g.seq_length
    anchors += [(0, 1), (0, NODE1), (L - 1, L), (L - 5, L), (0, L), (NODE1 - 1, NODE1 + 1), (g.pos(7, 1000), g.pos(8) + 1),
                (g.pos(8, 10000), g.pos(9) + 1), (g.pos(5), g.pos(5, 10) + 1), (g.pos(6, 99), g.pos(6, 99) + 1), (g.pos(2), g.pos(2) + 1),
                (g.pos(LAST_NODE - 1), L)]
    n = len(anchors)
    return build_case("decimal-edges", g, [(anchors, [[i] for i in range(n)] + [list(range(n))])])


def length_case(seed=5200):
    """every text length from 12 to 28 bytes; 200 anchors of mixed length in one chain, so that the exclusive prefix inside a
    round of 64 is not a multiple of anything; and a chain whose first round is all 28 bytes and whose second is all 12"""
    g, rng = digits_graph(), random.Random(seed)
    by_length = [_anchor_of_length(g, rng, n) for n in range(SHORTEST, LONGEST + 1)]
    mixed = [_anchor_of_length(g, rng, rng.randint(SHORTEST, LONGEST)) for _ in range(200)]
    long_short = [_anchor_of_length(g, rng, LONGEST) for _ in range(64)] + [_anchor_of_length(g, rng, SHORTEST) for _ in range(64)]
    n0, n1, n2 = len(by_length), len(mixed), len(long_short)
    return build_case("text-lengths", g, [
        (by_length, [list(range(n0))] + [[i] for i in range(n0)]),
        (mixed, [list(range(n1))]),
        (long_short, [list(range(n2)), list(range(64, n2)) + list(range(64))]),
    ])


def shape_case(seed=5300):
    """chains of every member count of MEMBER_COUNTS, over several reads with several chains each: members skip anchors and do
    not start at the read's first one, placeholders stand first, in the middle and last, one read has no anchors at all and
    another has anchors and only a placeholder"""
    g, rng = digits_graph(), random.Random(seed)
    reads = [([_random_anchor(g, rng) for _ in range(5)], [None])]
    counts = list(MEMBER_COUNTS)
    rng.shuffle(counts)
    for at in range(0, len(counts), 3):
        chains, n_anchors = [], 0
        for m in counts[at:at + 3]:
            gaps = [rng.randint(1, 3) for _ in range(m)]  # (>= 1: no chain starts at anchor 0 of its read)
            chains.append([n_anchors + sum(gaps[:i + 1]) for i in range(m)])
            n_anchors = chains[-1][-1] + 1 + rng.randint(0, 2)
        rng.shuffle(chains)
        reads.append(([_random_anchor(g, rng) for _ in range(n_anchors)], chains))
        if at == 3:
            reads.append(([], [None]))
    reads[2][1].insert(1, None)
    reads.append(([_random_anchor(g, rng) for _ in range(4)], [[1, 3], None]))
    return build_case("chain-shapes", g, reads)


def count_case(n_chains, seed=5400):
    """n_chains chains of 1 to 3 anchors, up to four chains a read"""
    g, rng = digits_graph(), random.Random(seed + n_chains)
    reads, left = [], n_chains
    while left:
        k = min(left, rng.randint(1, 4))
        chains, n_anchors = [], rng.randint(0, 2)
        for _ in range(k):
            m = rng.randint(1, 3)
            chains.append(list(range(n_anchors, n_anchors + m)))
            n_anchors += m + rng.randint(0, 1)
        reads.append(([_random_anchor(g, rng) for _ in range(n_anchors)], chains))
        left -= k
    return build_case("chains-%d" % n_chains, g, reads)


def no_chain_case():
    g = digits_graph()
    return build_case("no-chains", g, [([(0, 1)], []), ([], [])])


def placeholder_case(seed=5500):
    """every chain a placeholder: vga_chain_paths_text returns before its first launch, text_off all zero"""
    g, rng = digits_graph(), random.Random(seed)
    return build_case("only-placeholders", g, [([_random_anchor(g, rng) for _ in range(n)], [None]) for n in (0, 3, 1)])


@functools.lru_cache(maxsize=None)
def all_cases():
    return (edge_case(), length_case(), shape_case()) + tuple(count_case(n) for n in CHAIN_COUNTS) + (no_chain_case(), placeholder_case())


def case(name):
    return next(c for c in all_cases() if c.name == name)
