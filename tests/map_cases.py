"""Seeded mapping cases for the branches of k_kmer_probe / k_anchor_sort / k_chain4 / k_strand_pick (csrc/vga_map.hip) that
simulated reads reach by chance at best: exact score ties (the argmax takes the largest j among the tied lanes), anchor counts
around the 64-anchor load block, gaps of exactly max_gap at the size where the gap-cost table moves from LDS to HBM, graph
lengths at the edges of the sort's pass count, reads on both sides of the integer / f64 argmax threshold in one launch,
several chains on one maximum, strand ties.  Plain Python: no GPU, no oracle.

A case is `(nodes, edges, k, reads, params)`: node ids are consecutive from 1 (Graph.from_nodes_edges), every graph but one is a line
of nodes, `params` holds the vga_map_params fields that differ from the defaults (bandwidth 50, max_gap 1000,
chain_min_n_anchors 3, only_forward 1, strands forward).  `all_cases()` is the set tests/test_map_cases_gpu.py runs;
tests/test_map_cases_cpu.py shows from the oracle alone that each case produces the condition it is there for."""
import functools
import random
from collections import namedtuple

K = 11
MAX_GAP_LIMIT = 1 << 22  # the largest max_gap map_validate accepts
DEFAULTS = dict(bandwidth=50, max_gap=1000, chain_min_n_anchors=3, only_forward=1, strands=0)
STRANDS_BOTH = 1  # VGA_STRANDS_BOTH (include/vga_hip.h)

REPEAT_UNITS = ("A", 30), ("AC", 20), ("ACG", 15), (None, 20)  # None: a random 37-base unit
ANCHOR_COUNTS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
BANDWIDTHS = (1, 63, 64)
MIN_ANCHORS = (1, 3)
GAP_LIMITS = (0, 50, 2047, 2048)
SORT_LENGTHS = (255, 256, 257, 65535, 65536, 65537)

Case = namedtuple("Case", "name family nodes edges k reads params")


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rc(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def _distinct_kmers(s, k):
    return len({s[i:i + k] for i in range(len(s) - k + 1)}) == len(s) - k + 1


def _unique_seq(rng, n, k=K):
    """a random sequence without a repeated k-mer: an error-free read of it has one anchor per k-mer"""
    while True:
        s = _seq(rng, n)
        if _distinct_kmers(s, k):
            return s


def _line(seqs):
    seqs = [s for s in seqs if s]
    return [(i + 1, s) for i, s in enumerate(seqs)], [(i, i + 1) for i in range(1, len(seqs))]


def params_of(case):
    p = dict(DEFAULTS)
    p.update(case.params)
    return p


def linear_sequence(case):
    """the forward linearisation of the case's graph (its nodes form a line)"""
    return "".join(s for _, s in case.nodes)


def forward_anchor_count(case, read):
    """the number of forward anchors of a read: the occurrences of its k-mers in the line"""
    g, k = linear_sequence(case), case.k
    occ = {}
    for i in range(len(g) - k + 1):
        occ[g[i:i + k]] = occ.get(g[i:i + k], 0) + 1
    return sum(occ.get(read[i:i + k], 0) for i in range(len(read) - k + 1))


# ---------------------------------------------------------------- a. repeats
def repeat_cases(seed=4100):
    """flank - repeat - flank.  A read of the repeat has an anchor for every (read k-mer, period) pair: most steps of the DP see
    several predecessors with the same rounded score.  The reads: the repeat once, three times, and the left flank's second half
    running into the repeat.  With only_forward = 0 the reverse-strand records join in; AT x 20 is its own reverse complement."""
    out = []
    for n, (unit, times) in enumerate(REPEAT_UNITS + (("AT", 20),)):
        rng = random.Random(seed + n)
        unit = unit or _seq(rng, 37)
        rep = unit * times
        left, right = _seq(rng, 40), _seq(rng, 40)
        nodes, edges = _line([left, rep, right])
        reads = [rep, rep * 3, left[20:] + rep[:30]]
        tag = "%sx%d" % (unit if len(unit) < 4 else "unit%d" % len(unit), times)
        for fwd in (1, 0):
            if unit == "AT" and fwd:
                continue
            for ma in MIN_ANCHORS:
                out.append(Case("repeat-%s-%s-min%d" % (tag, "fwd" if fwd else "all", ma), "repeat", nodes, edges, K, reads,
                                dict(chain_min_n_anchors=ma, only_forward=fwd)))
    return out


# ---------------------------------------------------------------- b. anchor counts
def _substitute(s, positions):
    s = list(s)
    for p in positions:
        s[p] = {"A": "C", "C": "G", "G": "T", "T": "A"}[s[p]]
    return "".join(s)


def count_reads(node):
    """error-free reads of A + k - 1 bases for every A of ANCHOR_COUNTS (A anchors each: the node repeats no k-mer), then the
    same reads with a substitution at one third and at two thirds: the k-mers over them are lost and the chain has to jump"""
    clean = [node[100:100 + a + K - 1] for a in ANCHOR_COUNTS]
    return clean + [_substitute(s, (len(s) // 3, 2 * len(s) // 3)) for s in clean]


def count_cases(seed=4200):
    """the 64-anchor window of k_chain4 against the 64-anchor load blocks: anchor counts on both sides of 64, 128, 256, 512
    with the window at its widest (63, 64) and narrowest (1)"""
    node = _unique_seq(random.Random(seed), 2000)
    nodes, edges = _line([node])
    reads = count_reads(node)
    return [Case("count-bw%d-min%d" % (bw, ma), "count", nodes, edges, K, reads, dict(bandwidth=bw, chain_min_n_anchors=ma))
            for bw in BANDWIDTHS for ma in MIN_ANCHORS]


# ---------------------------------------------------------------- c. gap limits
def gap_cases(seed=4300):
    """X - Y - Z with the read X + Z: the first anchors of Z see the last anchors of X across a gap of exactly |Y|.  |Y| = max_gap
    reads gap_cost[max_gap] (the table's last entry; at 2048 the table is in HBM, at 2047 in LDS) and still pays, 400 matching
    bases against a cost of about 231 at most; |Y| = max_gap + 1 has to refuse the jump.  max_gap = 0: |Y| is 0 (no Y) or 1."""
    rng = random.Random(seed)
    while True:
        x, z = _seq(rng, 400), _seq(rng, 400)
        if _distinct_kmers(x + "N" + z, K):
            break

    def graph(ylen):  # Y shares no k-mer with the read, so no anchor of Y offers itself as a stepping stone
        yrng = random.Random(seed + 1 + ylen)
        while True:
            y = _seq(yrng, ylen)
            g = x + y + z
            in_graph = {g[i:i + K] for i in range(len(g) - K + 1)}
            hits = sum((x + z)[i:i + K] in in_graph for i in range(800 - K + 1))
            if len(in_graph) == len(g) - K + 1 and hits == (790 if ylen == 0 else 780):
                return _line([x, y, z])

    out = []
    for mg in GAP_LIMITS:
        for ylen in (mg, mg + 1):
            nodes, edges = graph(ylen)
            out.append(Case("gap-max%d-y%d" % (mg, ylen), "gap", nodes, edges, K, [x + z], dict(max_gap=mg)))
    nodes, edges = graph(50)
    out.append(Case("gap-max%d-y50" % MAX_GAP_LIMIT, "gap", nodes, edges, K, [x + z], dict(max_gap=MAX_GAP_LIMIT)))
    return out


# ---------------------------------------------------------------- d. sort key width
def sort_cases(seed=4400):
    """two nodes of L bases in all: k_anchor_sort's pass count follows the bit width of L, and the anchor on the last k-mer has
    target_end == L, the one key that needs the top bit at L = 256 and L = 65536.  The read of the last k bases has one anchor:
    with an odd pass count the kernel has to copy it to the buffer the host reads."""
    out = []
    for L in SORT_LENGTHS:
        rng = random.Random(seed + L)
        while True:
            s = _seq(rng, L)
            occ = {}
            for i in range(L - K + 1):
                occ[s[i:i + K]] = occ.get(s[i:i + K], 0) + 1
            if all(occ[s[i:i + K]] == 1 for i in list(range(30)) + list(range(L - 40, L - K + 1))):
                break
        nodes, edges = _line([s[:L // 3], s[L // 3:]])
        out.append(Case("sort-L%d" % L, "sort", nodes, edges, K, [s[-40:], s[-K:], s[:40]], {}))
    return out


# ---------------------------------------------------------------- e. both argmax paths in one launch
def key_anchors(k, max_gap):
    """map_call::chain() (csrc/vga_map.hip): reads with at most this many anchors take the argmax on 32-bit integers"""
    import math

    gc_last = 0.0 if max_gap == 0 else 0.01 * k * max_gap + 0.5 * math.log2(max_gap)
    room = 2147483647.0 / 1000.0 - gc_last - 4.0 * k - 16.0
    return int(min(room / k, 4.0e9)) if room > 0.0 else 0


def argmax_case(seed=4500):
    """k = 32 and the largest max_gap leave about 25 160 anchors for the integer argmax.  A 41-base unit x 30 gives a read of m
    units about 29 (41 m - 31) anchors: 10 units stay below the threshold, 25 and 29 go above it, and the short reads sit beside
    them in the same workgroups (four reads each)."""
    rng = random.Random(seed)
    unit = _seq(rng, 41)
    left, right = _unique_seq(rng, 50, 32), _unique_seq(rng, 50, 32)
    nodes, edges = _line([left, unit * 30, right])
    reads = [unit * 10, unit * 25, left, unit * 29, left[10:] + unit, unit * 2 + right]
    return Case("argmax-both-sides", "argmax", nodes, edges, 32, reads, dict(max_gap=MAX_GAP_LIMIT))


def argmax_sides(case):
    """per read: True when its anchor count is above key_anchors, i.e. the f64 argmax"""
    limit = key_anchors(case.k, params_of(case)["max_gap"])
    return [forward_anchor_count(case, r) > limit for r in case.reads]


# ---------------------------------------------------------------- f. equal-score chains
def equal_chain_case(seed=4600):
    """one 300-base piece twice, 1500 bases apart: a read of the piece chains equally well on either copy, and reads of two and
    three pieces leave anchors of one chain in the way of the next"""
    rng = random.Random(seed)
    while True:
        piece, spacer = _seq(rng, 300), _seq(rng, 1500)
        if _distinct_kmers(piece + "N" + spacer, K):
            break
    nodes, edges = _line([piece, spacer, piece])
    return Case("equal-chains", "equal", nodes, edges, K, [piece, piece * 2, piece * 3], {})


def shared_predecessor_cases(seed=4650):
    """P -> (a | b), both arms beginning with the same base, and the read P plus that base: its last k-mer has a record through
    either arm, both extend the last anchor of P by one base without a gap, so two anchors sit on the maximum and share their
    predecessor.  The chain that is found second meets anchors the first one consumed and stops there, two anchors long: kept
    with chain_min_n_anchors = 1, rolled back with 3 (after another chain was written)."""
    rng = random.Random(seed)
    while True:
        p, a, b = _seq(rng, 300), "G" + _seq(rng, 20), "G" + _seq(rng, 20)
        if _distinct_kmers(p + a, K) and _distinct_kmers(p + b, K) and a[1] != b[1]:
            break
    nodes, edges = [(1, p), (2, a), (3, b)], [(1, 2), (1, 3)]
    return [Case("equal-shared-predecessor-min%d" % ma, "equal", nodes, edges, K, [p + "G", p[150:] + "G", p], dict(chain_min_n_anchors=ma))
            for ma in MIN_ANCHORS]


# ---------------------------------------------------------------- g. strand ties
def strand_case(seed=4700):
    """S - spacer - rc(S): S, rc(S) and the palindrome S[:100] + rc(S[:100]) chain equally well as given and reverse
    complemented, and k_strand_pick has to keep them as given; the last read matches only as its reverse complement"""
    rng = random.Random(seed)
    while True:
        s, spacer = _seq(rng, 200), _seq(rng, 300)
        g = s + spacer + rc(s)
        if _distinct_kmers(s + "N" + spacer, K) and not any(rc(g[i:i + K]) in g for i in range(200, 500 - K + 1)):
            break
    nodes, edges = _line([s, spacer, rc(s)])
    reads = [s, rc(s), s[:100] + rc(s[:100]), rc(spacer[50:250])]
    return Case("strand-ties", "strand", nodes, edges, K, reads, dict(strands=STRANDS_BOTH))


STRAND_TIE_READS = (0, 1, 2)


@functools.lru_cache(maxsize=None)
def all_cases():
    return repeat_cases() + count_cases() + gap_cases() + sort_cases() + [argmax_case(), equal_chain_case()] + shared_predecessor_cases() + [strand_case()]


def cases(family):
    return [c for c in all_cases() if c.family == family]
