"""Reference walker for the pileup: the table of vga_pileup_read from the text of an alignments GAF, the node starts of the index
and its forward sequence, and from nothing else.  It shares no code with the product (test infrastructure).

Meaning, per aligned record (path column not "*"): walk the path (column 6, all ">") from offset path_start (column 8) inside
its first node along the cs string.  Per graph base seven counters, in the order of COLUMNS --
    :N    N graph bases, each adds one to the column of its own letter in seq_fwd
    *gq   one graph base, adds one to the column of q
    -g..  each of its graph bases adds one to del
    +q..  adds one to ins of the graph base consumed most recently before it (covered or deleted); with no base consumed yet it
          adds one to leading_ins and touches no base
-- moving to offset 0 of the next path node once the current one is used up.  A letter other than a c g t counts as N.  The
walker checks itself on every record: it must end exactly at path_end (column 9) on the last path node, the bases it covers
must equal block_length (column 11), and the g of every *gq and -g.. must be the lower-cased graph base where the walk stands."""
import re

import numpy as np

COLUMNS = ("A", "C", "G", "T", "N", "del", "ins")
DEL, INS = 5, 6
_CS = re.compile(r"(:[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+)")
_COL = {"a": 0, "c": 1, "g": 2, "t": 3}


def column(letter):
    return _COL.get(letter.lower(), 4)


def walk(gaf_text, node_seq_idx, seq_fwd):
    """-> (counts[seq_length, 7] uint32, n_alignments, leading_ins)"""
    idx = [int(x) for x in node_seq_idx]
    seq = seq_fwd.decode() if isinstance(seq_fwd, (bytes, bytearray)) else str(seq_fwd)
    assert len(seq) == idx[-1]
    counts = np.zeros((idx[-1], 7), dtype=np.int64)
    n_al = leading = 0
    for line in gaf_text.splitlines():
        f = line.split("\t")
        if len(f) < 12 or f[5] == "*":
            continue
        assert re.fullmatch(r"(>[0-9]+)+", f[5]), f[5]
        path = [int(x) for x in f[5][1:].split(">")]
        start, end, block = int(f[7]), int(f[8]), int(f[10])
        m = re.search(r"cs:Z:([^,\s]*)", "\t".join(f[11:]))
        assert m, line[:200]
        toks = _CS.findall(m.group(1))
        assert "".join(toks) == m.group(1), m.group(1)[:200]
        n_al += 1
        pi, off, covered, last = 0, start, 0, None
        for t in toks:
            if t[0] == "+":
                if last is None:
                    leading += 1
                else:
                    counts[last, INS] += 1
                continue
            # the graph bases of the token, one at a time: (what the cs says the graph holds or None, column)
            if t[0] == ":":
                items = [(None, None)] * int(t[1:])
            elif t[0] == "*":
                items = [(t[1], column(t[2]))]
            else:
                items = [(g, DEL) for g in t[1:]]
            for g, col in items:
                while off == idx[path[pi]] - idx[path[pi] - 1]:
                    pi, off = pi + 1, 0
                    assert pi < len(path), "the cs string runs past the path"
                pos = idx[path[pi] - 1] + off
                if g is not None:
                    assert g == seq[pos].lower(), ("the cs names another graph base", t, pos, seq[pos])
                counts[pos, column(seq[pos]) if col is None else col] += 1
                covered += col != DEL
                last = pos
                off += 1
        assert pi == len(path) - 1 and off == end, ("the walk must end at path_end on the last node", pi, len(path), off, end)
        assert covered == block, ("covered bases must equal block_length", covered, block)
    return counts.astype(np.uint32), n_al, leading


def cs_totals(gaf_text):
    """(summed length of the - tokens, number of + tokens) over the aligned records of a GAF text"""
    n_del = n_ins = 0
    for line in gaf_text.splitlines():
        f = line.split("\t")
        if len(f) < 12 or f[5] == "*":
            continue
        for t in _CS.findall(re.search(r"cs:Z:([^,\s]*)", "\t".join(f[11:])).group(1)):
            n_del += len(t) - 1 if t[0] == "-" else 0
            n_ins += t[0] == "+"
    return n_del, n_ins
