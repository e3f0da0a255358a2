"""Reference for path edit: the reads x paths matrix of vga_path_edit_last and the accumulators of vga_path_edit_read from the
text of an alignments GAF, the S and P lines of the GFA and the read sequences, and from nothing else.  It shares no code with the
product (test infrastructure).

The measure (include/vga_hip.h).  For the record reported for read r: the query Q of m letters is the read, or its reverse
complement for a '-' record; its node path is column 6.  Path p has the sequence seq_p: its steps' node sequences in order, an
"id-" step reverse-complemented (N stays N); pos_p(i) is the offset of step i.  Letters are compared upper-cased; A, C, G and T equal
themselves, anything else matches nothing.
    a = the first node of the record's path that p visits as "id+", i = the FIRST such step of p
    b = the last node of the record's path that p visits as "id+",  j = the LAST such step of p
    no such node, or j < i: NONE
    lo = max(0, pos_p(i) - m), hi = min(|seq_p|, pos_p(j) + len(b) + m)
    e[r][p] = min over lo <= s <= t <= hi of edit(Q, seq_p[s:t]), unit costs
A placeholder record has a NONE row; so has a read of more than `limit` letters, counted in n_too_long.

Two independent distances: dp_distance, a plain column-by-column dynamic programme (numpy over the rows of a column), and
myers_distance, Myers' bit-vector algorithm on one m-bit Python integer.  brute_distance is the definition itself, for tiny inputs."""
import numpy as np

NONE = 0xFFFFFFFF
LIMIT = 16384
FIELDS = ("n_scored", "sum_edit", "best", "best_alone")
_COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}


def code(c):
    """A C G T in either case -> 0..3, anything else -> -1"""
    return "ACGT".find(c.upper()) if len(c) == 1 else -1


def reverse_complement(s):
    return "".join(_COMPLEMENT.get(c, c) for c in reversed(s))


# ---------------------------------------------------------------------------------------------------------------- distances
def brute_distance(q, t):
    """the definition: the smallest full edit distance between q and any substring of t (the empty one included)"""
    def edit(a, b):
        prev = list(range(len(b) + 1))
        for i in range(1, len(a) + 1):
            cur = [i] + [0] * len(b)
            for j in range(1, len(b) + 1):
                same = code(a[i - 1]) >= 0 and code(a[i - 1]) == code(b[j - 1])
                cur[j] = min(prev[j - 1] + (0 if same else 1), prev[j] + 1, cur[j - 1] + 1)
            prev = cur
        return prev[len(b)]

    return min(edit(q, t[s:e]) for s in range(len(t) + 1) for e in range(s, len(t) + 1))


def dp_distance(q, t):
    """Sellers: the top row is 0, the answer the minimum of the bottom row (column 0 included).  A column at a time."""
    m = len(q)
    qa = np.array([code(c) for c in q], dtype=np.int64)
    ar = np.arange(m + 1, dtype=np.int64)
    col = ar.copy()
    best = int(col[m])
    for c in t:
        cc = code(c)
        sub = np.where(qa == cc, 0, 1) if cc >= 0 else np.ones(m, dtype=np.int64)
        new = np.empty(m + 1, dtype=np.int64)
        new[0] = 0
        new[1:] = np.minimum(col[:-1] + sub, col[1:] + 1)
        col = np.minimum.accumulate(new - ar) + ar  # (the vertical step: new[i] = min over k <= i of new[k] + (i - k))
        best = min(best, int(col[m]))
    return best


def myers_distance(q, t):
    """Myers 1999 with one m-bit word (a Python integer), the search variant: nothing is shifted into the horizontal deltas"""
    m = len(q)
    if m == 0:
        return 0
    mask = (1 << m) - 1
    top = 1 << (m - 1)
    peq = [0, 0, 0, 0]
    for i, c in enumerate(q):
        if code(c) >= 0:
            peq[code(c)] |= 1 << i
    pv, mv, score = mask, 0, m
    best = m
    for c in t:
        eq = peq[code(c)] if code(c) >= 0 else 0
        xv = eq | mv
        xh = ((((eq & pv) + pv) & mask) ^ pv) | eq
        ph = mv | (~(xh | pv) & mask)
        mh = pv & xh
        if ph & top:
            score += 1
        elif mh & top:
            score -= 1
        ph = (ph << 1) & mask
        mh = (mh << 1) & mask
        pv = mh | (~(xv | ph) & mask)
        mv = ph & xv
        if score < best:
            best = score
    return best


# ---------------------------------------------------------------------------------------------------------------- the rule
def parse_gfa(path):
    """-> ({node id: sequence}, [(name, [(node id, is_reverse), ...]), ...]) from the S and P lines"""
    node_seq, paths = {}, []
    for line in open(path):
        f = line.rstrip("\r\n").split("\t")
        if f[0] == "S":
            node_seq[int(f[1])] = f[2]
        elif f[0] == "P":
            paths.append((f[1], [(int(s[:-1]), s[-1] == "-") for s in f[2].split(",") if s]))
    return node_seq, paths


def path_sequence(steps, node_seq):
    """-> (seq_p, [pos_p(i) for every step])"""
    parts, pos, at = [], [], 0
    for node, rev in steps:
        s = node_seq[node]
        parts.append(reverse_complement(s) if rev else s)
        pos.append(at)
        at += len(s)
    return "".join(parts), pos


def window(record_nodes, steps, pos, node_seq, m, seq_len):
    """-> (lo, hi), or None where the pair is not scored"""
    forward = {}
    for i, (node, rev) in enumerate(steps):
        if not rev:
            forward.setdefault(node, []).append(i)
    on = [n for n in record_nodes if n in forward]
    if not on:
        return None
    a, b = on[0], on[-1]
    i, j = forward[a][0], forward[b][-1]
    if j < i:
        return None
    return max(0, pos[i] - m), min(seq_len, pos[j] + len(node_seq[b]) + m)


def records(gaf_text):
    """per GAF line: None for a placeholder, else (strand, [node ids])"""
    out = []
    for line in gaf_text.splitlines():
        if not line:
            continue
        f = line.split("\t")
        if len(f) < 12 or f[5] == "*":
            out.append(None)
            continue
        assert f[4] in "+-" and f[5][0] == ">" and "<" not in f[5], f[4:6]
        out.append((f[4], [int(x) for x in f[5][1:].split(">")]))
    return out


def windows(gaf_text, reads, gfa, limit=LIMIT):
    """-> [per GAF line: None (placeholder, too long), else (Q, [per path: None or (lo, hi)])], paths' sequences"""
    node_seq, paths = parse_gfa(gfa)
    seqs = [path_sequence(st, node_seq) for _, st in paths]
    recs = records(gaf_text)
    assert len(recs) == len(reads), (len(recs), len(reads))
    out = []
    for rec, read in zip(recs, reads):
        if rec is None or len(read) > limit:
            out.append(None)
            continue
        q = reverse_complement(read) if rec[0] == "-" else read
        out.append((q, [window(rec[1], st, pos, node_seq, len(q), len(seq)) for (_, st), (seq, pos) in zip(paths, seqs)]))
    return out, [s for s, _ in seqs]


def walk(gaf_text, reads, gfa, limit=LIMIT, distance=myers_distance):
    """-> dict: edit (int64 [GAF lines, paths], NONE where not scored), lengths (int64 [GAF lines]: m of the scored rows, else 0),
    n_scored, sum_edit, best, best_alone (int64 [paths]), n_alignments, n_too_long"""
    wins, seqs = windows(gaf_text, reads, gfa, limit)
    recs = records(gaf_text)
    P = len(seqs)
    out = dict(edit=np.full((len(wins), P), NONE, dtype=np.int64), lengths=np.zeros(len(wins), dtype=np.int64), n_alignments=0, n_too_long=0)
    for k in FIELDS:
        out[k] = np.zeros(P, dtype=np.int64)
    for r, w in enumerate(wins):
        if recs[r] is None:
            continue
        out["n_alignments"] += 1
        if w is None:
            out["n_too_long"] += 1
            continue
        q, per_path = w
        out["lengths"][r] = len(q)
        for p, lohi in enumerate(per_path):
            if lohi is not None:
                out["edit"][r, p] = distance(q, seqs[p][lohi[0]:lohi[1]])
        row = out["edit"][r]
        scored = np.flatnonzero(row != NONE)
        out["n_scored"][scored] += 1
        out["sum_edit"][scored] += row[scored]
        if len(scored):
            tops = scored[row[scored] == row[scored].min()]
            out["best"][tops] += 1
            if len(tops) == 1:
                out["best_alone"][tops[0]] += 1
    return out


def add(x, y):
    out = {k: x[k] + y[k] for k in FIELDS}
    out.update(n_alignments=x["n_alignments"] + y["n_alignments"], n_too_long=x["n_too_long"] + y["n_too_long"])
    return out


def likelihood_matrices(w):
    """the two matrices the likelihood reads from the edit distance: bases' = m - e (0 for NONE), edges' = 0"""
    e = w["edit"]
    b = np.where(e == NONE, 0, w["lengths"][:, None] - np.where(e == NONE, 0, e))
    return b.astype(np.uint64), np.zeros_like(b, dtype=np.uint64)


def same(got, want, what=""):
    for k in FIELDS:
        assert np.array_equal(np.asarray(got[k], dtype=np.int64), want[k]), (what, k, np.asarray(got[k]).tolist(), want[k].tolist())
    assert got["n_alignments"] == want["n_alignments"] and got["n_too_long"] == want["n_too_long"], (what, got["n_alignments"], got["n_too_long"])
