"""Seeded alignment cases for the three kernels that read a traceback's operations forward in blocks of 64 with one virtual
closing operation behind the last: k_poa_text (csrc/vga_poa_text.hpp: cs, CIGAR, node path), k_cov_runs (csrc/vga_coverage.hip)
and k_pu_events (csrc/vga_pileup.hip).  Simulated reads leave to chance which lane of a block an event lands on, never hold an
`=` run of 64, an insertion or deletion run that spans a block, or a run length of four digits.  Here they are planted.

The forward index f of an alignment column counts the columns before it; f % 64 is the lane that reads it.  The alignment is
global over the subgraph, and on the one-node graph DRB5 (12 856 bases) the subgraph is the node: the column of graph base p is
p plus the read bases inserted before it, so an Edit script puts every event on the lane it names.  On DRB1 the subgraph moves
with the read; there 64 reads at consecutive starts sweep every event kind over every lane.

A case set is `Case(name, graph, k, reads, both_strands)`; `graph` names the GFA (`gfa_path`).  The generator uses no GPU;
`alignments` takes the oracle as an argument and returns its alignments GAF of a set, `properties` derives from that text alone
what tests/test_op_cases_cpu.py asserts: that every condition the sets are there for is present in the oracle's alignments."""
import functools
import os
import re
from collections import namedtuple

K = 11
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
GRAPHS = {"drb5": os.path.join(DATA, "hla", "6-DRB5-3127.gfa"), "drb1": os.path.join(DATA, "DRB1-3123.gfa")}
SYNTH_BP, SYNTH_SEED = 20000, 78

Case = namedtuple("Case", "name graph k reads both_strands")
# one record of the oracle's alignments GAF: `cols` holds one (kind, graph letter, read letter) per alignment column with kind
# E (=), X, I or D; `cigar` the (length, letter) runs; `entries` the f of every graph-consuming column that enters a node, as
# (f, node id, adjacent): adjacent when the node follows the previous one on the linearised graph (ids are consecutive)
Record = namedtuple("Record", "name path path_start path_end cols cigar entries")

_CS = re.compile(r"(:[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+)")
_CG = re.compile(r"([0-9]+)([MID])")
_COMP = str.maketrans("ACGTN", "TGCAN")


def rc(s):
    return s[::-1].translate(_COMP)


def _other(*avoid):
    """a letter that is none of `avoid`"""
    return next(c for c in "ACGT" if c not in avoid)


# ---------------------------------------------------------------- graphs
def gfa_path(case, tmp_dir):
    """the GFA of a case set; the synthetic pangenome is written to tmp_dir on first use"""
    if case.graph != "synth":
        return GRAPHS[case.graph]
    out = os.path.join(str(tmp_dir), "op_cases_synth.gfa")
    if not os.path.exists(out):
        _readsim().synth_pangenome(out, SYNTH_BP, seed=SYNTH_SEED)
    return out


def _readsim():
    import __graft_entry__ as ge

    return ge.load_package().readsim


def node_lengths(gfa):
    return {int(f[1]): len(f[2]) for f in (ln.rstrip("\r\n").split("\t") for ln in open(gfa)) if f[0] == "S"}


@functools.lru_cache(maxsize=None)
def _path(graph, i):
    rs = _readsim()
    segs, paths = rs.parse_gfa_paths(GRAPHS[graph])
    return rs.path_sequence(segs, paths[i][1])


def _first_path(graph):
    return _path(graph, 0)


# ---------------------------------------------------------------- edit scripts on the one-node graph
class Edit:
    """A read of h[a:...] written event by event.  `ins` counts the bases inserted so far, so the column of graph base p is
    p + ins, and `at(lane, gap)` is the first graph position at least `gap` behind the last event whose column falls on `lane`."""

    def __init__(self, h, a, prefix=""):
        self.h, self.p, self.ins, self.out = h, a, len(prefix), [prefix]

    def at(self, lane, gap=40, ok=lambda p: True):
        p = self.p + gap
        while (p + self.ins) % 64 != lane % 64 or not ok(p):
            p += 1 if (p + self.ins) % 64 != lane % 64 else 64
        return p

    def copy_to(self, p):
        assert p >= self.p
        self.out.append(self.h[self.p:p])
        self.p = p

    def sub(self, lane, gap=40, letter=None):
        """a mismatch whose column is on `lane`: another letter, or `letter` (N)"""
        p = self.at(lane, gap)
        self.copy_to(p)
        self.out.append(letter or _other(self.h[p]))
        self.p = p + 1

    def insert(self, lane, n, gap=40, n_at=None):
        """n inserted bases, the first on `lane`, of a letter that neither neighbour holds (so the run cannot slide or match);
        n_at: that base of the run is N"""
        p = self.at(lane, gap)
        self.copy_to(p)
        run = [_other(self.h[p - 1], self.h[p])] * n
        if n_at is not None:
            run[n_at] = "N"
        self.out.append("".join(run))
        self.ins += n

    def delete(self, lane, n, gap=40):
        """n deleted graph bases, the first on `lane`, where the run cannot slide to either side"""
        h = self.h
        p = self.at(lane, gap, lambda p: h[p] != h[p + n] and h[p - 1] != h[p + n - 1])
        self.copy_to(p)
        self.p = p + n

    def read(self, b=None, gap=60, suffix=""):
        self.copy_to(self.p + gap if b is None else b)
        return "".join(self.out) + suffix


# ---------------------------------------------------------------- a. digits (DRB5)
LONG_LENGTHS = (9999, 10000, 10001)
DIGIT_STEPS = (9, 10, 99, 100, 999, 1000)


def digit_case():
    """exact reads h[100:100 + L] align as 100D <L>M <rest>D (four digits): L on both sides of 10 000.  One read holds `=` runs of
    9, 10, 99, 100, 999 and 1000 between one-base insertions, another deletion runs of 9, 10, 99 and 100
    (run_case has the insertion runs); a short exact read leaves a deletion run of five digits."""
    h = _first_path("drb5")
    reads = [h[100:100 + L] for L in LONG_LENGTHS]
    e = Edit(h, 200)
    e.insert(5, 1, gap=30)
    for n in DIGIT_STEPS:
        e.insert(e.p + e.ins + n, 1, gap=n)
    reads.append(e.read())
    e = Edit(h, 3000)
    for i, n in enumerate((9, 10, 99, 100)):
        e.delete(20 + i, n, gap=100)
    reads.append(e.read())
    reads.append(h[6000:6700])
    return Case("drb5-digits", "drb5", K, reads, False)


# ---------------------------------------------------------------- b. block edges (DRB5)
CLOSING = {0: 8, 1: 9, 63: 7}  # nops % 64 -> inserted bases: 12 856 = 200 * 64 + 56


def edge_case():
    h = _first_path("drb5")
    n = len(h)
    reads = []
    # the closing operation alone in its block, second in it, last in it; with them: a mismatch that closes an `=` run at lane
    # 0, mismatches at lane 63 and lane 0 inside one M run (apart, and side by side), N as the read base at lane 0 and 63
    e = Edit(h, 1000)
    e.sub(0, gap=200)
    e.insert(0, CLOSING[0], gap=130)  # (an insertion run at lane 0 directly behind a match)
    e.sub(63)
    e.sub(0, gap=64)
    e.sub(63, gap=64)
    e.sub(0, gap=0)
    reads.append(e.read())
    e = Edit(h, 2500)
    e.sub(0, gap=150, letter="N")
    e.sub(63, gap=70, letter="N")
    e.insert(17, CLOSING[1], n_at=4)  # (N inside an insertion)
    e.sub(62)
    e.sub(63, gap=0)
    e.sub(0, gap=0)
    e.sub(1, gap=0)
    reads.append(e.read())
    e = Edit(h, 4000)
    e.insert(63, CLOSING[63], gap=100)
    e.delete(0, 3)
    e.delete(63, 2)
    e.delete(61, 3)  # (ends at lane 63: the `=` behind it is at lane 0)
    reads.append(e.read())
    # deletion runs that hold whole blocks: from lane 0 to lane 63, and from lane 63 over two blocks.  (The band of the DP is
    # about 10 + 1 % of the read wide around the diagonals through the two ends of the subgraph, here the whole node: a short read
    # cannot insert more than a dozen bases.  run_case and sweep_case have the long insertion runs.)
    e = Edit(h, 5000)
    e.delete(0, 64, gap=100)
    e.delete(63, 130, gap=100)
    reads.append(e.read())
    # the ends: a leading insertion (a foreign prefix on a read of the first bases of the graph), a first `=`, a last insertion,
    # a last mismatch, a last `=`; every other read begins and ends with a deletion
    foreign = _other(h[0]) * 6
    reads.append(Edit(h, 0, prefix=foreign).read(b=700))
    reads.append(h[:640])
    e = Edit(h, n - 700)
    e.sub(63)
    reads.append(e.read(b=n, suffix=_other(h[-1]) * 6))
    reads.append(h[n - 600:n - 1] + _other(h[-1], h[-2]))
    e = Edit(h, n - 700)
    e.insert(20, CLOSING[0])  # (the closing operation at lane 0 behind an `=` run that fills the last block)
    reads.append(e.read(b=n))
    return Case("drb5-edges", "drb5", K, reads, False)


# ---------------------------------------------------------------- c. every event kind on every lane (DRB1)
SWEEP_START, SWEEP_READS = 600, 64


def sweep_reads(hap, start=SWEEP_START, n=SWEEP_READS):
    """read s starts at start + s and carries a mismatch, an N, a homopolymer insertion of 70 bases and a deletion of 70"""
    reads = []
    for s in range(n):
        a = start + s
        t = hap[a:a + 1300]
        p_snp, p_n, p_ins, p_del = 150, 300, 500, 800
        while t[p_del] == t[p_del + 70] or t[p_del - 1] == t[p_del + 69]:
            p_del += 1
        c = _other(t[p_ins - 1], t[p_ins])
        reads.append(t[:p_snp] + _other(t[p_snp]) + t[p_snp + 1:p_n] + "N" + t[p_n + 1:p_ins] + c * 70 + t[p_ins:p_del] + t[p_del + 70:])
    return reads


REPLACED_WINDOWS = ((7771, 48), (1604, 16))  # (offset in DRB1's first path, bases inserted before it: 0 .. this - 1)


def replaced_window_reads(hap):
    """36 path bases that lack a letter, replaced by 36 of that letter: nothing can match, and a deletion plus an insertion
    (2 (24 + 36)) cost less than 36 mismatches (4 * 36).  At these two windows the oracle writes the deletion first and the
    insertion directly behind it.  The subgraph starts at a node edge, so moving the read does not move the column; j bases
    inserted before the window do.  They go in at three places, at most 16 each (the chain survives that); the two windows'
    columns are 48 lanes apart, so 48 reads on one and 16 on the other put the insertion on every lane."""
    reads = []
    for i, n in REPLACED_WINDOWS:
        b = next(b for b in "ACGT" if b not in hap[i - 1:i + 37])
        for j in range(n):
            parts, left = [hap[i - 700:i - 550]], j
            for at in (i - 550, i - 400, i - 250):
                m = min(left, 16)
                left -= m
                parts += [_other(hap[at - 1], hap[at]) * m, hap[at:at + 150]]
            reads.append("".join(parts) + hap[i - 100:i] + b * 36 + hap[i + 36:i + 636])
    return reads


def sweep_case():
    hap = _first_path("drb1")
    return Case("drb1-sweep", "drb1", K, sweep_reads(hap) + replaced_window_reads(hap), False)


# ---------------------------------------------------------------- d. long insertion runs (DRB1)
INSERT_RUNS = ((500, 9), (507, 10), (514, 99), (521, 100), (528, 130), (506, 64), (505, 70))  # (offset in the read, length)


def run_case():
    """DRB1's subgraph ends where the chain ends, and there the band follows an insertion of any length: runs on both sides of
    two and three digits, one that holds a whole block wherever it starts, one that is a block (the subgraph of these reads
    starts six bases before them: offset 506 is lane 0), one from lane 63 on, and a leading insertion"""
    hap = _first_path("drb1")
    t = hap[600:1900]
    reads = [t[:at] + _other(t[at - 1], t[at]) * m + t[at:] for at, m in INSERT_RUNS]
    # a leading insertion: a foreign prefix on a read of the first bases of the graph (the sixth path starts at node 1; the
    # first starts at node 8, where the subgraph still reaches back to node 7)
    first = _path("drb1", 5)
    reads.append(_other(first[0]) * 6 + first[:1000])
    return Case("drb1-runs", "drb1", K, reads, False)


# ---------------------------------------------------------------- e. many node entries in a block (DRB1)
def densest_window(graph="drb1", width=64):
    """(offset in the first path, nodes entered) of the `width` path bases that enter the most nodes"""
    rs = _readsim()
    segs, paths = rs.parse_gfa_paths(GRAPHS[graph])
    starts, off = [], 0
    for nid, _ in paths[0][1]:
        starts.append(off)
        off += len(segs[nid])
    best, j = (0, 0), 0
    for i, s in enumerate(starts):
        while starts[j] < s - width + 1:
            j += 1
        best = max(best, (i - j + 1, starts[j]))
    return best[1], best[0]


def entry_case():
    """exact reads over the stretch of DRB1's first path with the most node entries per 64 bases, at 16 starts four apart, so
    that one of them has the stretch inside a block"""
    hap = _first_path("drb1")
    off, _ = densest_window()
    return Case("drb1-entries", "drb1", K, [hap[off - 300 - 4 * s:off + 400 - 4 * s] for s in range(16)], False)


# ---------------------------------------------------------------- f. 32-bp nodes (synthetic pangenome)
def synth_case(tmp_dir):
    gfa = gfa_path(Case("", "synth", K, (), False), tmp_dir)
    rs = _readsim()
    reads = [r.seq for r in rs.simulate_reads(gfa, 12, 400, 0.0, 0.0, 0.0, seed=5)]
    reads += [r.seq for r in rs.simulate_reads(gfa, 12, 600, 0.03, 0.03, 0.04, seed=6)]
    return Case("synth-nodes", "synth", K, reads, False)


# ---------------------------------------------------------------- g. both strands (DRB1)
def strand_case():
    """sixteen of the sweep's reads, every other one given as its reverse complement (for strands = BOTH)"""
    reads = sweep_reads(_first_path("drb1"), start=2000, n=16)
    return Case("drb1-both-strands", "drb1", K, [rc(r) if i % 2 else r for i, r in enumerate(reads)], True)


def all_cases(tmp_dir):
    return [digit_case(), edge_case(), run_case(), sweep_case(), entry_case(), synth_case(tmp_dir), strand_case()]


BLOCK_EDGE_SETS = ("drb5-digits", "drb5-edges", "drb1-runs")  # the sets the routes of tests/test_op_cases_gpu.py run on


# ---------------------------------------------------------------- the oracle's side
def forward_reads(case):
    """the reads in the orientation that aligns forward: what the oracle, which maps one strand, is given"""
    return [rc(r) if case.both_strands and i % 2 else r for i, r in enumerate(case.reads)]


def alignments(oracle, index, case):
    """the oracle's alignments GAF of a case set (one line per read, in order)"""
    reads = forward_reads(case)
    return oracle.map_reads(index, ["r%d" % i for i in range(len(reads))], reads)[1]


Aligned = namedtuple("Aligned", "case gfa index gaf records")


def oracle_side(oracle, tmp_dir):
    """name -> Aligned: every case set with its GFA, the oracle's index, its alignments GAF and the records' properties"""
    out = {}
    for c in all_cases(tmp_dir):
        gfa = gfa_path(c, tmp_dir)
        ix = oracle.Index(oracle.Graph.from_gfa(gfa), c.k)
        gaf = alignments(oracle, ix, c)
        out[c.name] = Aligned(c, gfa, ix, gaf, properties(gaf, node_lengths(gfa)))
    return out


def properties(gaf_text, node_len):
    """one Record per aligned line of an alignments GAF (None for a placeholder), from the text and the node lengths alone"""
    out = []
    for line in gaf_text.splitlines():
        f = line.split("\t")
        if f[5] == "*":
            out.append(None)
            continue
        path = [int(x) for x in f[5][1:].split(">")]
        m = re.search(r"cs:Z:([^,\s]*),cg:Z:(\S+)", "\t".join(f[11:]))
        toks = _CS.findall(m.group(1))
        assert "".join(toks) == m.group(1)
        cols = []
        for t in toks:
            if t[0] == ":":
                cols += [("E", None, None)] * int(t[1:])
            elif t[0] == "*":
                cols.append(("X", t[1], t[2]))
            elif t[0] == "+":
                cols += [("I", None, c) for c in t[1:]]
            else:
                cols += [("D", c, None) for c in t[1:]]
        cigar = [(int(n), c) for n, c in _CG.findall(m.group(2))]
        assert "".join("%d%s" % rc_ for rc_ in cigar) == m.group(2)
        assert sum(n for n, _ in cigar) == len(cols)
        entries, pi, off = [], 0, int(f[7])
        for i, (kind, _, _) in enumerate(cols):
            if kind == "I":
                continue
            if not entries:
                entries.append((i, path[0], False))
            while off == node_len[path[pi]]:
                pi, off = pi + 1, 0
                entries.append((i, path[pi], path[pi] == path[pi - 1] + 1))
            off += 1
        assert pi == len(path) - 1 and off == int(f[8])
        assert len(entries) == len(path) and len({e[0] for e in entries}) == len(path), "an empty node on the path"
        out.append(Record(f[0], path, int(f[7]), int(f[8]), cols, cigar, entries))
    return out


def runs(rec):
    """the maximal runs of equal column kinds of a record: (kind, first f, length)"""
    out, i = [], 0
    while i < len(rec.cols):
        j = i
        while j < len(rec.cols) and rec.cols[j][0] == rec.cols[i][0]:
            j += 1
        out.append((rec.cols[i][0], i, j - i))
        i = j
    return out
