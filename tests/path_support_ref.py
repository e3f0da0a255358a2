"""Reference walker for path support: the reads x paths tables of vga_path_support_last and the accumulators of
vga_path_support_read from the text of an alignments GAF and the S and P lines of the GFA, and from nothing else.  It shares no
code with the product (test infrastructure); the GAF records are parsed by coverage_ref.records.

Meaning, per aligned record r (path column not "*") and path p of the GFA (steps "id+" / "id-"): walk r's path (column 6, all ">")
from offset path_start (column 8) inside its first node along the cs string --
    :N    N graph bases, covered
    *gq   one graph base, covered
    -g..  its graph bases are skipped
    +q..  touches no graph base
-- moving to offset 0 of the next path node once the current one is used up.
    bases[r][p]  covered bases that lie in a node p visits as "id+" (a node p visits twice counts once, an "id-" step nothing)
    edges[r][p]  consecutive pairs (a, b) of r's path for which p has the step a+ immediately followed by b+
The top paths of r are those whose key (bases, edges) is the lexicographic maximum, unless the maximum is (0, 0).  A placeholder
record has a zero row and adds nothing.  The walker checks itself on every record as coverage_ref.walk does: it must end exactly
at path_end (column 9) on the last path node, and the bases it covers must equal block_length (column 11)."""
import numpy as np

import coverage_ref


def parse_gfa(path):
    """-> ({node id: length}, [(name, [(node id, is_reverse), ...]), ...]) from the S and P lines"""
    node_len, paths = {}, []
    for line in open(path):
        f = line.rstrip("\r\n").split("\t")
        if f[0] == "S":
            node_len[int(f[1])] = len(f[2])
        elif f[0] == "P":
            steps = [(int(s[:-1]), s[-1] == "-") for s in f[2].split(",") if s]
            assert all(s[-1] in "+-" for s in f[2].split(",") if s)
            paths.append((f[1], steps))
    return node_len, paths


def packed_steps(paths):
    """(step_off, steps) as Context.path_support_begin takes them"""
    off = np.zeros(len(paths) + 1, dtype=np.uint64)
    steps = []
    for i, (_, st) in enumerate(paths):
        steps += [(n << 1) | (1 if rev else 0) for n, rev in st]
        off[i + 1] = len(steps)
    return off, np.asarray(steps, dtype=np.uint64)


def covered_per_node(path, start, end, block, toks, node_len):
    """covered bases of every node of a record's path, in path order (with the two self-checks)"""
    cov = [0] * len(path)
    pi, off = 0, start
    for t in toks:
        if t[0] == "+":
            continue
        count, cover = (int(t[1:]), True) if t[0] == ":" else (1, True) if t[0] == "*" else (len(t) - 1, False)
        while count:
            ln = node_len[path[pi]]
            if off == ln:
                pi, off = pi + 1, 0
                assert pi < len(path), "the cs string runs past the path"
                continue
            step = min(count, ln - off)
            if cover:
                cov[pi] += step
            off += step
            count -= step
    assert pi == len(path) - 1 and off == end, ("the walk must end at path_end on the last node", pi, len(path), off, end)
    assert sum(cov) == block, ("covered bases must equal block_length", sum(cov), block)
    return cov


def walk(gaf_text, node_len, paths):
    """-> dict: bases, edges (int64 [GAF lines, paths]; a placeholder line has a zero row), sum_bases, sum_edges, top, top_alone
    (int64 [paths]), n_alignments, n_unplaced, top_paths (per line the list of its top paths)"""
    fwd = [{n for n, rev in st if not rev} for _, st in paths]
    pairs = [{(a[0], b[0]) for a, b in zip(st, st[1:]) if not a[1] and not b[1]} for _, st in paths]
    lines = [ln for ln in gaf_text.splitlines() if ln]
    P = len(paths)
    out = dict(bases=np.zeros((len(lines), P), dtype=np.int64), edges=np.zeros((len(lines), P), dtype=np.int64),
               sum_bases=np.zeros(P, dtype=np.int64), sum_edges=np.zeros(P, dtype=np.int64), top=np.zeros(P, dtype=np.int64),
               top_alone=np.zeros(P, dtype=np.int64), n_alignments=0, n_unplaced=0, top_paths=[[] for _ in lines])
    for r, line in enumerate(lines):
        recs = coverage_ref.records(line)
        if not recs:
            continue
        path, start, end, block, toks = recs[0]
        cov = covered_per_node(path, start, end, block, toks, node_len)
        for p in range(P):
            out["bases"][r, p] = sum(c for n, c in zip(path, cov) if n in fwd[p])
            out["edges"][r, p] = sum(1 for ab in zip(path, path[1:]) if ab in pairs[p])
        keys = [(int(out["bases"][r, p]), int(out["edges"][r, p])) for p in range(P)]
        best = max(keys)
        out["n_alignments"] += 1
        if best == (0, 0):
            out["n_unplaced"] += 1
        else:
            tops = [p for p in range(P) if keys[p] == best]
            out["top_paths"][r] = tops
            for p in tops:
                out["top"][p] += 1
            if len(tops) == 1:
                out["top_alone"][tops[0]] += 1
        out["sum_bases"] += out["bases"][r]
        out["sum_edges"] += out["edges"][r]
    return out
