"""Reference for the insertion table and the insertion call: what vga_insertion_read / vga_insertion_call /
vga_insertion_call_table return and what <out>-insertions.tsv holds, from the text of an alignments GAF, the node starts of the
index and its forward sequence, and from nothing else.  Written from the definition in include/vga_hip.h with Python integers; it
shares no code with the product (test infrastructure).

Walk the record reported for a read exactly as the pileup does (pileup_ref.walk).  A cs token "+q.." of L letters belongs to the
graph base consumed most recently before it, covered or deleted; one before the first consumed base adds one to n_leading and
touches no counter.  Per graph base COLS = 49 counters:
    columns 0 .. 8          len[1] .. len[8], len_more: the insertions at the base of exactly l letters, of more than 8
    column 9 + 5 j + c      let[j][A C G T N], j = 0 .. 7: the insertions at the base of more than j letters whose j-th letter
                            is that one (anything but a c g t is N); a longer insertion adds its first 8 letters
The walker checks itself on every record as pileup_ref.walk does, and asserts against pileup_ref.walk on the same text that the
bins of a base add up to the pileup's ins there, that the five letters of position j add up to the insertions longer than j, and
that n_leading is the pileup's leading_ins.

The call of a row: length = the bin with the most reads among 1 .. 8, more (the shorter on a tie, more being the longest and
reported as 9; 0 for a row without insertions); for j < min(length, 8) the letter with the largest count, A < C < G < T < N on a
tie."""
import re

import numpy as np

import pileup_ref

MAX_LEN = 8
BINS = MAX_LEN + 1
LETTERS = "ACGTN"
COLS = BINS + MAX_LEN * len(LETTERS)
MORE = MAX_LEN + 1  # the length a call reports for `more`
HEADER = "node\toffset\tstate\tins_qual\tdepth\tins_count\tlength\tlength_reads\tseq\tseq_reads"
INS_STATES = (".", "het", "hom")
_CS = re.compile(r"(:[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+)")


def len_col(length):
    return min(length, MORE) - 1


def let_col(j, letter):
    return BINS + len(LETTERS) * j + pileup_ref.column(letter)


def walk(gaf_text, node_seq_idx, seq_fwd):
    """-> (counts[seq_length, 49] uint32, n_alignments, n_events, n_leading)"""
    idx = [int(x) for x in node_seq_idx]
    seq = seq_fwd.decode() if isinstance(seq_fwd, (bytes, bytearray)) else str(seq_fwd)
    assert len(seq) == idx[-1]
    counts = np.zeros((idx[-1], COLS), dtype=np.int64)
    n_al = n_ev = leading = 0
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
                    continue
                run = t[1:]
                n_ev += 1
                counts[last, len_col(len(run))] += 1
                for j, letter in enumerate(run[:MAX_LEN]):
                    counts[last, let_col(j, letter)] += 1
                continue
            n = int(t[1:]) if t[0] == ":" else 1 if t[0] == "*" else len(t) - 1
            for i in range(n):
                while off == idx[path[pi]] - idx[path[pi] - 1]:
                    pi, off = pi + 1, 0
                    assert pi < len(path), "the cs string runs past the path"
                last = idx[path[pi] - 1] + off
                if t[0] == "*":
                    assert t[1] == seq[last].lower(), ("the cs names another graph base", t, last)
                elif t[0] == "-":
                    assert t[1 + i] == seq[last].lower(), ("the cs names another graph base", t, last)
                covered += t[0] != "-"
                off += 1
        assert pi == len(path) - 1 and off == end, ("the walk must end at path_end on the last node", pi, len(path), off, end)
        assert covered == block, ("covered bases must equal block_length", covered, block)
    # the three invariants, against the pileup's walker on the same text
    pu, pu_al, pu_leading = pileup_ref.walk(gaf_text, idx, seq)
    assert n_al == pu_al and leading == pu_leading, (n_al, pu_al, leading, pu_leading)
    bins = counts[:, :BINS].sum(1)
    assert np.array_equal(bins, pu[:, pileup_ref.INS].astype(np.int64)), "the bins of a base add up to the pileup's ins"
    assert int(bins.sum()) == n_ev
    check_rows(counts)
    return counts.astype(np.uint32), n_al, n_ev, leading


def check_rows(counts):
    """the letters of position j add up to the insertions of more than j letters"""
    c = np.asarray(counts).astype(object).reshape(-1, COLS)
    for j in range(MAX_LEN):
        longer = c[:, j:BINS].sum(1)  # len[l] is column l - 1
        assert (c[:, BINS + 5 * j:BINS + 5 * j + 5].sum(1) == longer).all(), ("letters of position", j)


def call_row(row):
    """one row -> (length 0 .. 9, length_reads, seq: str of min(length, 8) letters, seq_reads: list)"""
    row = [int(v) for v in row]
    assert len(row) == COLS
    length, reads = 0, 0
    for b in range(BINS):  # ascending: a later bin wins only when strictly larger
        if row[b] > reads:
            length, reads = b + 1, row[b]
    seq, seq_reads = "", []
    for j in range(min(length, MAX_LEN)):
        let = row[BINS + 5 * j:BINS + 5 * j + 5]
        best = let.index(max(let))  # the first maximum: A < C < G < T < N
        seq += LETTERS[best]
        seq_reads.append(let[best])
    return length, reads, seq, seq_reads


def call_rows(rows):
    """-> the dict Context.insertion_call_table returns: length, length_reads, seq[n, 8] (bytes, 0 behind the last letter),
    seq_reads[n, 8], rows"""
    rows = [[int(v) for v in r] for r in np.asarray(rows, dtype=object).reshape(-1, COLS).tolist()]
    n = len(rows)
    out = {"length": np.zeros(n, dtype=np.uint8), "length_reads": np.zeros(n, dtype=np.uint64), "seq": np.zeros((n, MAX_LEN), dtype=np.uint8),
           "seq_reads": np.zeros((n, MAX_LEN), dtype=np.uint64), "rows": np.array(rows, dtype=np.uint64).reshape(n, COLS)}
    for i, r in enumerate(rows):
        length, reads, seq, seq_reads = call_row(r)
        out["length"][i], out["length_reads"][i] = length, reads
        for j, (c, v) in enumerate(zip(seq, seq_reads)):
            out["seq"][i, j], out["seq_reads"][i, j] = ord(c), v
    return out


def same(a, b):
    """two result dicts agree exactly; returns the name of the first field that differs, or None"""
    for k in ("length", "length_reads", "seq", "seq_reads", "rows"):
        if np.asarray(a[k]).shape != np.asarray(b[k]).shape or not np.array_equal(np.asarray(a[k]).astype(object), np.asarray(b[k]).astype(object)):
            return k
    return None


def tsv(variant_calls, counts, node_seq_idx):
    """the text of <out>-insertions.tsv: the sites of a variant_ref result dict whose insertion state is het or hom, in that
    order, called from the insertion table `counts`; -> (text, sites, sites longer than 8)"""
    idx = np.asarray([int(x) for x in node_seq_idx], dtype=np.int64)
    lines, n_long = [HEADER], 0
    for j in range(len(variant_calls["pos"])):
        state = int(variant_calls["ins"][j])
        if state not in (1, 2):
            continue
        p = int(variant_calls["pos"][j])
        node = int(np.searchsorted(idx, p, side="right"))
        length, reads, seq, seq_reads = call_row(counts[p])
        n_long += length > MAX_LEN
        f = [node, p - int(idx[node - 1]), INS_STATES[state], int(variant_calls["ins_qual"][j]), int(variant_calls["depth"][j]),
             int(variant_calls["counts"][j][pileup_ref.INS]), ">%d" % MAX_LEN if length > MAX_LEN else length, reads, seq or ".",
             ",".join(str(v) for v in seq_reads) or "."]
        lines.append("\t".join(str(v) for v in f))
    return "\n".join(lines) + "\n", len(lines) - 1, n_long


def tsv_gaf(gaf_text, node_seq_idx, seq_fwd, **variant_parameters):
    """the same from the alignments GAF alone"""
    import variant_ref

    calls = variant_ref.call_gaf(gaf_text, node_seq_idx, seq_fwd, **variant_parameters)
    return tsv(calls, walk(gaf_text, node_seq_idx, seq_fwd)[0], node_seq_idx)
