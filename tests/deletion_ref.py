"""Reference for the deletion call: the events of vga_deletion_read, the calls of vga_deletion_call and <out>-deletions.tsv from the
text of an alignments GAF, the node starts of the index and the pileup table (tests/pileup_ref.py), and from nothing else.  Python
integers only; it shares no code with the product (test infrastructure).

Run.  The record reported for a read is walked exactly as pileup_ref.walk walks it.  A run is one "-g.." token of cs: len its
letters, first and last the positions in seq_fwd of its first and last deleted base.  No two "-" tokens are adjacent (a run is a
maximal sequence of D operations): the walker asserts it.

End run.  A run with no ":" or "*" token before it in the record, or none behind it.  It is counted in n_end_runs and otherwise
ignored.  Every other run is an event (first, len, last), kept in the order of the records and then along the record.

Call.  The events sorted by (first, len, last) and grouped: reads the size of a group, depth = A + C + G + T + N + del of the
pileup row at first.  With k = min(reads, depth) and the error cost E:  none costs k E,  het 256 depth,  hom (depth - k) E;  the
first minimum in that order is the state, qual the second smallest cost minus the smallest, saturated at 2^32 - 1.  A group is
reported when depth >= min_depth, the state is not none and qual >= min_qual.

The invariant check_against_pileup asserts: for every base, the events that start there number at most the pileup's del there."""
import re
from collections import Counter

import numpy as np

EVENT_WORDS = 3
STATES = ("none", "het", "hom")
NONE, HET, HOM = range(3)
QUAL_MAX = 2**32 - 1
ERROR, MIN_DEPTH, MIN_QUAL = 1280, 4, 512   # the defaults of --call-variants
HEADER = "node\toffset\tend_node\tend_offset\tlength\tstate\tqual\tdepth\treads"
_CS = re.compile(r"(:[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+)")
DEL = 5


def record_runs(toks, path, start, idx):
    """one record: the runs [(first, len, last, is_end)] along it; idx are the node starts, path the node ids, start the offset in
    the first node"""
    out, pi, off = [], 0, start
    m_at = [i for i, t in enumerate(toks) if t[0] in ":*"]
    for i, t in enumerate(toks):
        if t[0] == "+":
            continue
        n = int(t[1:]) if t[0] == ":" else 1 if t[0] == "*" else len(t) - 1
        if t[0] == "-":
            assert i == 0 or toks[i - 1][0] != "-", "two adjacent - tokens"
        first = last = None
        for _ in range(n):
            while off == idx[path[pi]] - idx[path[pi] - 1]:
                pi, off = pi + 1, 0
            last = idx[path[pi] - 1] + off
            if first is None:
                first = last
            off += 1
        if t[0] == "-":
            is_end = not m_at or i < m_at[0] or i > m_at[-1]
            out.append((first, n, last, is_end))
    return out


def walk(gaf_text, node_seq_idx):
    """-> (events[n, 3] uint32 in store order, n_alignments, n_end_runs)"""
    idx = [int(x) for x in node_seq_idx]
    events, n_al, n_end = [], 0, 0
    for line in gaf_text.splitlines():
        f = line.split("\t")
        if len(f) < 12 or f[5] == "*":
            continue
        path = [int(x) for x in f[5][1:].split(">")]
        cs = re.search(r"cs:Z:([^,\s]*)", "\t".join(f[11:])).group(1)
        toks = _CS.findall(cs)
        assert "".join(toks) == cs
        n_al += 1
        for first, n, last, is_end in record_runs(toks, path, int(f[7]), idx):
            if is_end:
                n_end += 1
            else:
                events.append((first, n, last))
    return np.array(events, dtype=np.uint32).reshape(-1, EVENT_WORDS), n_al, n_end


def rule(reads, depth, error=ERROR):
    """-> (state, qual)"""
    reads, depth, error = int(reads), int(depth), int(error)
    k = min(reads, depth)
    costs = [k * error, 256 * depth, (depth - k) * error]
    state = costs.index(min(costs))   # the first minimum in the order none, het, hom
    ordered = sorted(costs)
    return state, min(ordered[1] - ordered[0], QUAL_MAX)


def depth_at(counts, pos):
    return sum(int(v) for v in counts[pos][:DEL + 1])


def call(events, counts, error=ERROR, min_depth=MIN_DEPTH, min_qual=MIN_QUAL):
    """events: rows (first, len, last); counts: the pileup table [n_bases, 7] -> the reported groups in sort order, as the dict the
    binding returns"""
    groups = Counter((int(a), int(b), int(c)) for a, b, c in np.asarray(events).reshape(-1, EVENT_WORDS).tolist())
    rows = []
    for key in sorted(groups):
        reads, depth = groups[key], depth_at(counts, key[0])
        state, qual = rule(reads, depth, error)
        if depth >= min_depth and state != NONE and qual >= min_qual:
            rows.append(key + (state, qual, depth, reads))
    col = lambda j, dt: np.array([r[j] for r in rows], dtype=dt)
    return {"first": col(0, np.uint32), "len": col(1, np.uint32), "last": col(2, np.uint32), "state": col(3, np.uint8), "qual": col(4, np.uint32),
            "depth": col(5, np.uint64), "reads": col(6, np.uint64), "n_distinct": len(groups), "n_calls": len(rows)}


FIELDS = ("first", "len", "last", "state", "qual", "depth", "reads")


def same(got, want, upto=None):
    """None when two results agree (in the first `upto` calls when given), else the name of the first field that differs"""
    for k in ("n_distinct", "n_calls"):
        if int(got[k]) != int(want[k]):
            return k
    for k in FIELDS:
        g, w = np.asarray(got[k]), np.asarray(want[k])[:upto]
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(g, w):
            return k
    return None


def check_against_pileup(events, counts):
    """for every base, the events starting there number at most the pileup's del there"""
    starts = Counter(int(e[0]) for e in np.asarray(events).reshape(-1, EVENT_WORDS).tolist())
    for pos, n in starts.items():
        assert n <= int(counts[pos][DEL]), (pos, n, int(counts[pos][DEL]))


def node_of(pos, idx):
    lo, hi = 1, len(idx)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if idx[mid - 1] <= pos:
            lo = mid
        else:
            hi = mid
    return lo


def tsv(calls, node_seq_idx):
    idx = [int(x) for x in node_seq_idx]
    lines = [HEADER]
    for i in range(int(calls["n_calls"])):
        first, last = int(calls["first"][i]), int(calls["last"][i])
        a, b = node_of(first, idx), node_of(last, idx)
        lines.append("\t".join(str(v) for v in (a, first - idx[a - 1], b, last - idx[b - 1], int(calls["len"][i]), STATES[int(calls["state"][i])],
                                                int(calls["qual"][i]), int(calls["depth"][i]), int(calls["reads"][i]))))
    return "\n".join(lines) + "\n"


def tsv_gaf(gaf_text, node_seq_idx, seq_fwd, error=ERROR, min_depth=MIN_DEPTH, min_qual=MIN_QUAL):
    """an alignments GAF -> (the text of <out>-deletions.tsv, the stderr line of `vgaligner map --call-deletions`, the calls)"""
    import pileup_ref

    events, n_al, n_end = walk(gaf_text, node_seq_idx)
    counts = pileup_ref.walk(gaf_text, node_seq_idx, seq_fwd)[0]
    check_against_pileup(events, counts)
    calls = call(events, counts, error, min_depth, min_qual)
    message = "call-deletions: %d runs of %d alignments, %d at an end, %d distinct, %d calls" % (len(events) + n_end, n_al, n_end, calls["n_distinct"], calls["n_calls"])
    return tsv(calls, node_seq_idx), message, calls
