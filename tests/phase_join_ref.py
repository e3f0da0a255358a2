"""Reference for the phase join: what vga_phase_set_links / vga_phase_set_links_lists / vga_phase_join return and what
<out>-phase-joined.tsv, <out>-phase-sets.tsv and <out>-phase-joins.tsv hold, from the observations of tests/phase_ref.py, the rows of
tests/haplotag_ref.py and the ps and flip of the phase chain, and from nothing else.  Written from the definition in
include/vga_hip.h with Python integers; it shares no code with the product (test infrastructure).

Sets: the distinct ps in ascending order, numbered 0 .. S - 1.  tag(r, s) is the hap of the haplotag row (r, s): a for votes_a >
votes_b, b for votes_b > votes_a, nothing on a tie or without a row.  table[pair_index(S, s, t)][2 i + j], s <= t, counts the reads
with tag(r, s) = i and tag(r, t) = j (0 = a, 1 = b).

The join keeps, instead of a union-find, a component label and a parity per set and relabels a whole component when two are joined:
a link is accepted exactly when the labels of its ends differ at its turn."""
import numpy as np

import haplotag_ref
import phase_ref

MIN_READS = 2
MAX_SETS = 4096
SETS_HEADER = "ps\tsites\treads_a\treads_b\tjoined_ps\tflip"
JOINS_HEADER = "ps_a\tps_b\tcis\ttrans\trel"


def pair_index(n, s, t):
    assert 0 <= s <= t < n
    return s * n - s * (s - 1) // 2 + (t - s)


def set_names(ps):
    return sorted(set(int(p) for p in ps))


def tags(obs, ps, flip):
    """-> per read {set index: 0 for a, 1 for b}"""
    at = {p: k for k, p in enumerate(set_names(ps))}
    out = [dict() for _ in obs]
    for r, p, a, b in haplotag_ref.rows(obs, ps, flip):
        if a != b:
            out[r][at[p]] = 0 if a > b else 1
    return out


def table(obs, ps, flip):
    """-> table[S (S + 1) / 2, 4] uint32"""
    S = len(set_names(ps))
    t = np.zeros((S * (S + 1) // 2, 4), dtype=np.int64)
    if len(obs) == 0:   # an empty store: zero rows
        return np.zeros((0, 4), dtype=np.uint32)
    for tagged in tags(obs, ps, flip):
        sets = sorted(tagged)
        for i, s in enumerate(sets):
            for u in sets[i:]:
                t[pair_index(S, s, u), 2 * tagged[s] + tagged[u]] += 1
    return t.astype(np.uint32)


def join(tbl, n_sets, min_reads=MIN_READS):
    """-> (set_root, set_flip, joins [(s, t, cis, trans)], agreeing, conflicting)"""
    S = int(n_sets)
    n = [[int(v) for v in row] for row in np.asarray(tbl).reshape(-1, 4).tolist()]
    assert len(n) == S * (S + 1) // 2 and 1 <= min_reads <= 65535
    links = []
    for s in range(S):
        for t in range(s + 1, S):
            r = n[pair_index(S, s, t)]
            cis, trans = r[0] + r[3], r[1] + r[2]
            if cis != trans and abs(cis - trans) >= min_reads:
                links.append((-abs(cis - trans), s, t, cis, trans))
    label, parity = list(range(S)), [0] * S   # label: the smallest set of the component; parity: against that set
    joins, agree, conflict = [], 0, 0
    for _, s, t, cis, trans in sorted(links):
        rel = int(trans > cis)
        if label[s] == label[t]:
            if parity[s] ^ parity[t] == rel:
                agree += 1
            else:
                conflict += 1
            continue
        keep, gone = min(label[s], label[t]), max(label[s], label[t])
        # the component that loses its name is turned so that the link holds: parity[s] ^ parity[t] = rel afterwards
        turn = parity[s] ^ parity[t] ^ rel
        for k in range(S):
            if label[k] == gone:
                label[k], parity[k] = keep, parity[k] ^ turn
        joins.append((s, t, cis, trans))
    assert all(parity[label[k]] == 0 and label[k] <= k for k in range(S))
    return label, parity, joins, agree, conflict


def sites(ps, flip, set_root, set_flip):
    """-> (ps', flip') per site"""
    names = set_names(ps)
    at = {p: k for k, p in enumerate(names)}
    return [names[set_root[at[int(p)]]] for p in ps], [int(f) ^ set_flip[at[int(p)]] for p, f in zip(ps, flip)]


def check_sets(ps):
    """what the library demands of a ps: 1 <= ps[h] <= h + 1, and ps[h] names a site that opens its set"""
    return all(1 <= p <= h + 1 and ps[p - 1] == p for h, p in enumerate(ps))


def joined_tsv(pos, x, y, links, site_reads, node_seq_idx, ps2, flip2, min_links=phase_ref.MIN_LINKS):
    """the text of <out>-phase-joined.tsv: the lines of <out>-phase.tsv with ps and gt from ps' and flip'"""
    text, _, _ = phase_ref.tsv(pos, x, y, links, site_reads, node_seq_idx, min_links)
    lines = text.splitlines()
    out = [lines[0]]
    for h, line in enumerate(lines[1:]):
        f = line.split("\t")
        a, b = (y[h], x[h]) if flip2[h] else (x[h], y[h])
        f[2], f[3] = phase_ref.ALLELES[int(a)] + "|" + phase_ref.ALLELES[int(b)], str(ps2[h])
        out.append("\t".join(f))
    return "\n".join(out) + "\n"


def sets_tsv(ps, tbl, set_root, set_flip):
    names = set_names(ps)
    S = len(names)
    t = np.asarray(tbl).reshape(-1, 4)
    lines = [SETS_HEADER]
    for k, p in enumerate(names):
        d = t[pair_index(S, k, k)] if len(t) else [0, 0, 0, 0]
        lines.append("%d\t%d\t%d\t%d\t%d\t%d" % (p, sum(1 for q in ps if int(q) == p), d[0], d[3], names[set_root[k]], set_flip[k]))
    return "\n".join(lines) + "\n"


def joins_tsv(ps, joins):
    names = set_names(ps)
    return "\n".join([JOINS_HEADER] + ["%d\t%d\t%d\t%d\t%s" % (names[s], names[t], cis, trans, "trans" if trans > cis else "cis") for s, t, cis, trans in joins]) + "\n"


def stderr_line(n_sets, joins, agree, conflict):
    return "phase-join: %d sets, %d joins, %d sets left, %d agreeing, %d conflicting links" % (n_sets, len(joins), n_sets - len(joins), agree, conflict)


def gaf(gaf_text, node_seq_idx, seq_fwd, min_links=phase_ref.MIN_LINKS, min_reads=MIN_READS, **variant_parameters):
    """everything from the alignments GAF alone -> dict"""
    import variant_ref

    calls = variant_ref.call_gaf(gaf_text, node_seq_idx, seq_fwd, **variant_parameters)
    pos, x, y = phase_ref.sites_of(calls)
    obs = phase_ref.observations(gaf_text, node_seq_idx, seq_fwd, pos, x, y)
    links, sr = phase_ref.tables(obs, len(pos))
    ps, flip, _ = phase_ref.chain(links, min_links)
    S = len(set_names(ps))
    tbl = table(obs, ps, flip)
    full = tbl if len(tbl) else np.zeros((S * (S + 1) // 2, 4), dtype=np.uint32)
    root, sflip, joins, agree, conflict = join(full, S, min_reads)
    ps2, flip2 = sites(ps, flip, root, sflip)
    return dict(pos=pos, x=x, y=y, obs=obs, links=links, site_reads=sr, ps=ps, flip=flip, n_sets=S, table=tbl, set_root=root, set_flip=sflip, joins=joins,
                agree=agree, conflict=conflict, ps2=ps2, flip2=flip2, calls=calls,
                joined_tsv=joined_tsv(pos, x, y, links, sr, node_seq_idx, ps2, flip2, min_links), sets_tsv=sets_tsv(ps, full, root, sflip),
                joins_tsv=joins_tsv(ps, joins), stderr=stderr_line(S, joins, agree, conflict))
