"""Reference for the haplotype paths: what vga_haplotype_paths / vga_haplotype_paths_lists / vga_haplotype_paths_store /
vga_haplotype_paths_rank return and what <out>-haplotype-paths.tsv holds, from the reads x paths matrices of
tests/path_support_ref.py or tests/path_edit_ref.py, the observations of tests/phase_ref.py, the rows of tests/haplotag_ref.py and
the ps and flip of the phase chain (or of the phase join), and from nothing else.  Written from the definition in
include/vga_hip.h with Python integers; it shares no code with the product (test infrastructure).

Kept reads: the aligned records of the GAF in order.  s[r][p] = bases[r][p] + edges[r][p]; d[r][p] = min(max_p' s[r][p'] - s[r][p],
cap); read r is scored when its maximum is above 0.  Sets: the distinct ps ascending, numbered 0 .. S - 1.  Group 2 s + h (h: 0 = a,
1 = b) holds the scored reads whose haplotag row (r, s) has more votes for h.  reads[g]: their number; table[g][p] = (sum of
d[r][p], number of r with d[r][p] = 0)."""
import numpy as np

import haplotag_ref
import phase_ref

CAP = 64
MAX_SETS = 4096
MAX_ENTRIES = 1 << 23
HEADER = "ps\thap\treads\trank\tpath\tcost\tmargin\tbest\ttied"


def set_names(ps):
    return sorted(set(int(p) for p in ps))


def deficits(bases, edges, cap=CAP):
    """-> (d uint8[n, P], scored uint8[n]) from two matrices of non-negative integers (any width: summed as Python integers)"""
    assert 1 <= cap <= 255
    b, e = np.asarray(bases), np.asarray(edges)
    assert b.shape == e.shape and b.ndim == 2
    d, scored = np.zeros(b.shape, dtype=np.uint8), np.zeros(len(b), dtype=np.uint8)
    for r in range(len(b)):
        s = [int(x) + int(y) for x, y in zip(b[r].tolist(), e[r].tolist())]
        m = max(s) if s else 0
        scored[r] = 1 if m > 0 else 0
        d[r] = [min(m - v, cap) for v in s]
    return d, scored


def tags(obs, ps, flip):
    """-> per read {set index: 0 for a, 1 for b}"""
    at = {p: k for k, p in enumerate(set_names(ps))}
    out = [dict() for _ in obs]
    for r, p, a, b in haplotag_ref.rows(obs, ps, flip):
        if a != b:
            out[r][at[p]] = 0 if a > b else 1
    return out


def sums(obs, ps, flip, d, scored):
    """-> (reads uint64[2 S], table uint64[2 S, P, 2]); an empty store or no site: zero groups"""
    d = np.asarray(d)
    P = d.shape[1]
    S = len(set_names(ps))
    if len(obs) == 0 or S == 0:
        return np.zeros(0, dtype=np.uint64), np.zeros((0, P, 2), dtype=np.uint64)
    assert len(obs) == len(d) == len(scored)
    reads = [0] * (2 * S)
    cost = [[0] * P for _ in range(2 * S)]
    best = [[0] * P for _ in range(2 * S)]
    for r, tagged in enumerate(tags(obs, ps, flip)):
        if not int(scored[r]):
            continue
        row = [int(v) for v in d[r].tolist()]
        for s, h in tagged.items():
            g = 2 * s + h
            reads[g] += 1
            for p, v in enumerate(row):
                cost[g][p] += v
                best[g][p] += 1 if v == 0 else 0
    table = np.zeros((2 * S, P, 2), dtype=np.uint64)
    table[:, :, 0] = np.array(cost, dtype=np.uint64).reshape(2 * S, P)
    table[:, :, 1] = np.array(best, dtype=np.uint64).reshape(2 * S, P)
    return np.array(reads, dtype=np.uint64), table


def rank(cost_best):
    """the rank rule restated: -> (order, tied): the paths by cost ascending, then in P-line order; the paths at the minimum"""
    cost = [int(row[0]) for row in cost_best]   # (Python integers throughout: a cost is 64 bits wide)
    order = sorted(range(len(cost)), key=lambda p: (cost[p], p))
    return order, sum(1 for c in cost if c == min(cost)) if cost else 0


def same(got_reads, got_table, want_reads, want_table, what=""):
    assert got_reads.dtype == np.uint64 and got_table.dtype == np.uint64, what
    assert got_reads.shape == want_reads.shape and got_table.shape == want_table.shape, (what, got_reads.shape, want_reads.shape, got_table.shape, want_table.shape)
    assert np.array_equal(got_reads, want_reads), (what, got_reads.tolist(), want_reads.tolist())
    bad = np.argwhere(got_table != want_table)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got_table[tuple(bad[:8].T)].tolist(), want_table[tuple(bad[:8].T)].tolist())


def tsv(ps, reads, table, path_names, top=5):
    """the text of <out>-haplotype-paths.tsv and the two stderr lines -> (text, [stderr lines])"""
    names = set_names(ps)
    lines = [HEADER]
    ranked = {}
    for g in range(len(reads)):
        if int(reads[g]) == 0:
            continue
        order, tied = rank(table[g])
        ranked[g] = (order, tied)
        c0 = int(table[g][order[0]][0])
        for k, p in enumerate(order if not top else order[:top]):
            lines.append("%d\t%s\t%d\t%d\t%s\t%d\t%d\t%d\t%d" % (names[g // 2], "ab"[g & 1], int(reads[g]), k + 1, path_names[p], int(table[g][p][0]),
                                                                 int(table[g][p][0]) - c0, int(table[g][p][1]), tied))
    return "\n".join(lines) + "\n", ranked


def stderr_lines(ps, reads, table, path_names, n_scored, n_kept):
    names = set_names(ps)
    S = len(reads) // 2
    _, ranked = tsv(ps, reads, table, path_names)
    out = ["haplotype-paths: %d sets, %d groups with reads, %d of %d kept reads scored" % (S, len(ranked), n_scored, n_kept)]
    if not ranked:
        return out + ["haplotype-paths: no call"]
    s = max(range(S), key=lambda k: (int(reads[2 * k]) + int(reads[2 * k + 1]), -k))

    def side(g):
        if g not in ranked:
            return ".", 0, 0
        order, tied = ranked[g]
        margin = int(table[g][order[1]][0]) - int(table[g][order[0]][0]) if len(order) > 1 else 0
        return path_names[order[0]], margin, tied
    (na, ma, ta), (nb, mb, tb) = side(2 * s), side(2 * s + 1)
    out.append("haplotype-paths: ps %d: %s | %s (reads %d | %d, margins %d | %d, tied %d | %d)" % (names[s], na, nb, int(reads[2 * s]), int(reads[2 * s + 1]), ma, mb,
                                                                                                  ta, tb))
    return out


def matrices(gaf_text, gfa, read_seqs=None, source="support"):
    """the two matrices of the kept reads (the aligned records of the text, in order) -> (bases, edges, path names)"""
    import path_edit_ref
    import path_support_ref

    kept = [i for i, line in enumerate(l for l in gaf_text.splitlines() if l) if len(line.split("\t")) >= 12 and line.split("\t")[5] != "*"]
    if source == "support":
        node_len, paths = path_support_ref.parse_gfa(gfa)
        w = path_support_ref.walk(gaf_text, node_len, paths)
        b, e = w["bases"], w["edges"]
    else:
        assert source == "edit" and read_seqs is not None
        _, paths = path_edit_ref.parse_gfa(gfa)
        b, e = path_edit_ref.likelihood_matrices(path_edit_ref.walk(gaf_text, read_seqs, gfa))
    return np.asarray(b)[kept], np.asarray(e)[kept], [name for name, _ in paths]


def gaf(gaf_text, gfa, node_seq_idx, seq_fwd, read_seqs=None, cap=CAP, source="support", top=5, join=False, min_links=phase_ref.MIN_LINKS, **variant_parameters):
    """everything from the alignments GAF and the GFA alone -> dict"""
    import phase_join_ref
    import variant_ref

    calls = variant_ref.call_gaf(gaf_text, node_seq_idx, seq_fwd, **variant_parameters)
    pos, x, y = phase_ref.sites_of(calls)
    obs = phase_ref.observations(gaf_text, node_seq_idx, seq_fwd, pos, x, y)
    links, _ = phase_ref.tables(obs, len(pos))
    ps, flip, _ = phase_ref.chain(links, min_links)
    if join:
        S = len(set_names(ps))
        tbl = phase_join_ref.table(obs, ps, flip)
        full = tbl if len(tbl) else np.zeros((S * (S + 1) // 2, 4), dtype=np.uint32)
        root, sflip, _, _, _ = phase_join_ref.join(full, S)
        ps, flip = phase_join_ref.sites(ps, flip, root, sflip)
    b, e, names = matrices(gaf_text, gfa, read_seqs, source)
    assert len(b) == len(obs)
    d, scored = deficits(b, e, cap)
    reads, table = sums(obs, ps, flip, d, scored)
    text, ranked = tsv(ps, reads, table, names, top)
    return dict(pos=pos, x=x, y=y, obs=obs, ps=ps, flip=flip, n_sets=len(reads) // 2, deficits=d, scored=scored, reads=reads, table=table, names=names, tsv=text,
                ranked=ranked, stderr=stderr_lines(ps, reads, table, names, int(scored.sum()), len(obs)), calls=calls, bases=b, edges=e)
