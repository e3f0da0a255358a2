"""Reference for the haplotype tags: what vga_phase_tags / vga_phase_tags_lists return and what <out>-haplotag.tsv holds, from
the observations of tests/phase_ref.py (observations: from the text of an alignments GAF; obs_lists: from stored lists) plus the ps
and flip of the phase chain, and from nothing else.  Written from the definition in include/vga_hip.h with Python integers; it
shares no code with the product (test infrastructure).

obs[r][h] is 0 for x alone, 1 for y alone, 2 consumed otherwise, 3 not consumed.  Site h votes in read r when obs[r][h] <= 1; its
vote is obs xor flip[h], 0 for haplotype a and 1 for haplotype b.  votes_a[r][p] and votes_b[r][p] count the votes of the sites
with ps[h] = p.  A row (read, ps, votes_a, votes_b) exists for every (r, p) with a vote; rows come by read, then by ps ascending.
hap is a for votes_a > votes_b, b for votes_b > votes_a and . on a tie."""
import numpy as np

import phase_ref

HEADER = "read\tps\thap\tvotes_a\tvotes_b"


def rows(obs, ps, flip):
    """-> [(read, ps, votes_a, votes_b)], read the index of the row of obs"""
    out = []
    for r, row in enumerate(obs):
        assert len(row) == len(ps) == len(flip)
        votes = {}
        for h, o in enumerate(row):
            if o <= 1:
                votes.setdefault(int(ps[h]), [0, 0])[o ^ int(flip[h])] += 1
        out += [(r, p, votes[p][0], votes[p][1]) for p in sorted(votes)]
    return out


def table(obs, ps, flip):
    """the same as the uint32 array the library returns"""
    return np.array(rows(obs, ps, flip), dtype=np.uint32).reshape(-1, 4)


def hap(votes_a, votes_b):
    return "a" if votes_a > votes_b else "b" if votes_b > votes_a else "."


def tsv(tag_rows, read_ids=None):
    """the text of <out>-haplotag.tsv; read_ids[r]: the number of record r's read in the input file (default: r itself)
    -> (text, rows, a, b, undecided)"""
    lines, n = [HEADER], {"a": 0, "b": 0, ".": 0}
    named = sorted((int(read_ids[r]) if read_ids is not None else int(r), int(p), int(a), int(b)) for r, p, a, b in tag_rows)
    for r, p, a, b in named:
        n[hap(a, b)] += 1
        lines.append("%d\t%d\t%s\t%d\t%d" % (r, p, hap(a, b), a, b))
    return "\n".join(lines) + "\n", len(named), n["a"], n["b"], n["."]


def tsv_gaf(gaf_text, node_seq_idx, seq_fwd, min_links=phase_ref.MIN_LINKS, **variant_parameters):
    """the same from the alignments GAF alone (one line per read of the input file, in its order; a read without an alignment is
    no record but keeps its number) -> (text, rows, a, b, undecided, records)"""
    import variant_ref

    calls = variant_ref.call_gaf(gaf_text, node_seq_idx, seq_fwd, **variant_parameters)
    pos, x, y = phase_ref.sites_of(calls)
    obs = phase_ref.observations(gaf_text, node_seq_idx, seq_fwd, pos, x, y)
    links, _ = phase_ref.tables(obs, len(pos))
    ps, flip, _ = phase_ref.chain(links, min_links)
    ids = [i for i, line in enumerate(gaf_text.splitlines()) if len(line.split("\t")) >= 12 and line.split("\t")[5] != "*"]
    assert len(ids) == len(obs)
    return tsv(rows(obs, ps, flip), ids) + (len(obs),)
