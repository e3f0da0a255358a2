"""Reference walker for read coverage: the four tables of vga_coverage_read from the text of an alignments GAF and the graph
arrays of the index, and from nothing else.  It shares no code with the product (test infrastructure).

Meaning, per aligned record (path column not "*"): walk the path (column 6, all ">") from offset path_start (column 8)
inside its first node along the cs string --
    :N    N graph bases, each  base_depth += 1
    *gq   one graph base,      base_depth += 1
    -g..  its graph bases are skipped
    +q..  touches no graph base
-- moving to offset 0 of the next path node once the current one is used up.  Every node of the path adds one to node_reads,
every consecutive pair (a, b) one to the slot of b in the outgoing part of a's edge slice.  The walker checks itself on every
record: it must end exactly at path_end (column 9) on the last path node, and the bases it covers must equal block_length
(column 11)."""
import re

import numpy as np

_CS = re.compile(r"(:[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+)")


def records(gaf_text):
    """the aligned records of a GAF text: (path node ids, path_start, path_end, block_length, cs tokens)"""
    out = []
    for line in gaf_text.splitlines():
        f = line.split("\t")
        if len(f) < 12 or f[5] == "*":
            continue
        assert re.fullmatch(r"(>[0-9]+)+", f[5]), f[5]
        path = [int(x) for x in f[5][1:].split(">")]
        m = re.search(r"cs:Z:([^,\s]*)", "\t".join(f[11:]))
        assert m, line[:200]
        toks = _CS.findall(m.group(1))
        assert "".join(toks) == m.group(1), m.group(1)[:200]
        out.append((path, int(f[7]), int(f[8]), int(f[10]), toks))
    return out


def walk(gaf_text, node_seq_idx, node_edge_idx, node_edges_to, edges):
    """-> (base_depth[seq_length], node_reads[n_nodes], edge_reads[n_edges], n_alignments), uint32 arrays"""
    idx = [int(x) for x in node_seq_idx]
    eidx = [int(x) for x in node_edge_idx]
    eto = [int(x) for x in node_edges_to]
    edg = [int(x) for x in edges]
    n_nodes = len(idx) - 1
    base = np.zeros(idx[-1], dtype=np.int64)
    node = np.zeros(n_nodes, dtype=np.int64)
    edge = np.zeros(len(edg), dtype=np.int64)
    n_al = 0
    for path, start, end, block, toks in records(gaf_text):
        n_al += 1
        pi, off, covered = 0, start, 0

        def take(count, cover):
            nonlocal pi, off, covered
            while count:
                ln = idx[path[pi]] - idx[path[pi] - 1]
                if off == ln:
                    pi, off = pi + 1, 0
                    assert pi < len(path), "the cs string runs past the path"
                    continue
                step = min(count, ln - off)
                if cover:
                    p0 = idx[path[pi] - 1] + off
                    base[p0:p0 + step] += 1
                    covered += step
                off += step
                count -= step

        for t in toks:
            if t[0] == ":":
                take(int(t[1:]), True)
            elif t[0] == "*":
                take(1, True)
            elif t[0] == "-":
                take(len(t) - 1, False)
        assert pi == len(path) - 1 and off == end, ("the walk must end at path_end on the last node", pi, len(path), off, end)
        assert covered == block, ("covered bases must equal block_length", covered, block)
        assert len(set(path)) == len(path)
        for a in path:
            assert 1 <= a <= n_nodes
            node[a - 1] += 1
        for a, b in zip(path, path[1:]):
            lo, hi = eidx[a - 1] + eto[a - 1], eidx[a]
            slots = [s for s in range(lo, hi) if edg[s] == 2 * b]
            assert slots, f"no edge {a} -> {b} in the index"
            edge[slots[0]] += 1
    return base.astype(np.uint32), node.astype(np.uint32), edge.astype(np.uint32), n_al


def outgoing_slots(node_edge_idx, node_edges_to, n_edges):
    """boolean mask over the edge array: True where a slot belongs to the outgoing part of its node's slice"""
    mask = np.zeros(n_edges, dtype=bool)
    for i in range(len(node_edge_idx) - 1):
        mask[int(node_edge_idx[i]) + int(node_edges_to[i]):int(node_edge_idx[i + 1])] = True
    return mask
