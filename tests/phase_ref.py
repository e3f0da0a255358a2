"""Reference for the phase links and the phase chain: what vga_phase_links / vga_phase_links_lists / vga_phase_chain return and
what <out>-phase.tsv holds, from the text of an alignments GAF, the node starts of the index, its forward sequence and the rows of
the variant call, and from nothing else.  Written from the definition in include/vga_hip.h with Python integers; it shares no
code with the product (test infrastructure).

Sites: the variant calls whose base genotype is heterozygous (x < y in A < C < G < T < D), in the order of the file.  A call that
is reported only for its insertion state is no site.

Observation of a record at site h: walk the record exactly as pileup_ref.walk does.  At graph base pos_h a ":N" that covers it
observes the base's own letter, "*gq" observes q (anything but a c g t is "other"), "-g.." observes D, a "+q.." observes nothing.
With sx = some observation equals x and sy likewise: obs = 0 for sx and not sy, 1 for sy and not sx, 2 when the base is consumed
otherwise, 3 when it is not consumed.

links[h][d - 1][2 a + b], 1 <= d <= WINDOW, h + d < H: the records with obs a at h and obs b at h + d (a, b in 0, 1);
site_reads[h] = the records with obs 0, 1, 2.

The same observations can be made from stored lists (obs_lists): per read run-event words in pairs (start << 1 covers start,
end << 1 | 1 does not cover end) and sparse words position << 3 | column (0 .. 3 A C G T, 4 another letter, 5 deleted, 6 an
insertion: ignored), with ref[h] the own letter of site h (4: none of A C G T, a run then observes "other")."""
import re

import numpy as np

import pileup_ref

WINDOW = 8
MIN_LINKS = 2
ALLELES = "ACGT-"
D, OTHER = 4, 5
HEADER = "node\toffset\tgt\tps\tlink\tcis\ttrans\tx_reads\ty_reads\tother_reads"
_CS = re.compile(r"(:[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+)")
_CODE = {"a": 0, "c": 1, "g": 2, "t": 3}


def allele(letter):
    return _CODE.get(letter.lower(), OTHER)


def sites_of(calls):
    """the heterozygous calls of a variant_ref result dict -> (pos, x, y) lists, in the order of the file"""
    keep = [j for j in range(len(calls["pos"])) if int(calls["x"][j]) < int(calls["y"][j])]
    return [int(calls["pos"][j]) for j in keep], [int(calls["x"][j]) for j in keep], [int(calls["y"][j]) for j in keep]


def _obs(seen, x, y):
    """the alleles one record has observed at one site -> 0 .. 3"""
    if not seen:
        return 3
    sx, sy = x in seen, y in seen
    return 0 if sx and not sy else 1 if sy and not sx else 2


def observations(gaf_text, node_seq_idx, seq_fwd, pos, x, y):
    """-> obs[n_records][H], the aligned records of the text in order"""
    idx = [int(v) for v in node_seq_idx]
    seq = seq_fwd.decode() if isinstance(seq_fwd, (bytes, bytearray)) else str(seq_fwd)
    site_at = {int(p): h for h, p in enumerate(pos)}
    assert len(site_at) == len(pos) and list(pos) == sorted(pos), "sites ascend strictly"
    out = []
    for line in gaf_text.splitlines():
        f = line.split("\t")
        if len(f) < 12 or f[5] == "*":
            continue
        assert re.fullmatch(r"(>[0-9]+)+", f[5]), f[5]
        path = [int(v) for v in f[5][1:].split(">")]
        start, end = int(f[7]), int(f[8])
        cs = re.search(r"cs:Z:([^,\s]*)", "\t".join(f[11:])).group(1)
        toks = _CS.findall(cs)
        assert "".join(toks) == cs
        seen = {}
        pi, off = 0, start
        for t in toks:
            if t[0] == "+":
                continue
            if t[0] == ":":
                items = [None] * int(t[1:])
            elif t[0] == "*":
                items = [allele(t[2])]
            else:
                items = [D] * (len(t) - 1)
            for a in items:
                while off == idx[path[pi]] - idx[path[pi] - 1]:
                    pi, off = pi + 1, 0
                p = idx[path[pi] - 1] + off
                if p in site_at:
                    seen.setdefault(site_at[p], set()).add(allele(seq[p]) if a is None else a)
                off += 1
        assert pi == len(path) - 1 and off == end, "the walk must end at path_end on the last node"
        out.append([_obs(seen.get(h), int(x[h]), int(y[h])) for h in range(len(pos))])
    return out


def obs_lists(recs, words, pos, x, y, ref):
    """the same from stored lists -> obs[n_reads][H]"""
    site_at = {int(p): h for h, p in enumerate(pos)}
    out = []
    for off, n_runs, n_sparse in [[int(v) for v in r] for r in recs]:
        seen = {}
        ev = [int(w) for w in words[off:off + n_runs]]
        for i in range(0, n_runs, 2):
            assert ev[i] & 1 == 0 and ev[i + 1] & 1 == 1
            for p in range(ev[i] >> 1, ev[i + 1] >> 1):
                if p in site_at:
                    h = site_at[p]
                    seen.setdefault(h, set()).add(int(ref[h]) if int(ref[h]) < 4 else OTHER)
        for w in [int(w) for w in words[off + n_runs:off + n_runs + n_sparse]]:
            p, col = w >> 3, w & 7
            if col == 6 or p not in site_at:
                continue
            seen.setdefault(site_at[p], set()).add(col if col < 4 else D if col == 5 else OTHER)
        out.append([_obs(seen.get(h), int(x[h]), int(y[h])) for h in range(len(pos))])
    return out


def tables(obs, n_sites):
    """-> (links[H, 8, 4] uint32, site_reads[H, 3] uint32)"""
    H = int(n_sites)
    links, sr = np.zeros((H, WINDOW, 4), dtype=np.int64), np.zeros((H, 3), dtype=np.int64)
    for row in obs:
        assert len(row) == H
        for h in range(H):
            if row[h] < 3:
                sr[h, row[h]] += 1
            if row[h] > 1:
                continue
            for d in range(1, WINDOW + 1):
                if h + d < H and row[h + d] <= 1:
                    links[h, d - 1, 2 * row[h] + row[h + d]] += 1
    return links.astype(np.uint32), sr.astype(np.uint32)


def chain(links, min_links=MIN_LINKS):
    """-> (ps, flip, link_d) lists; ps numbers a set by the 1-based line of the site that opens it"""
    ln = [[[int(v) for v in l] for l in site] for site in np.asarray(links).reshape(-1, WINDOW, 4).tolist()]
    ps, flip, link_d = [], [], []
    for h in range(len(ln)):
        for d in range(1, min(WINDOW, h) + 1):
            l = ln[h - d][d - 1]
            cis, trans = l[0] + l[3], l[1] + l[2]
            if cis != trans and abs(cis - trans) >= min_links:
                ps.append(ps[h - d]); flip.append(flip[h - d] ^ int(trans > cis)); link_d.append(d)
                break
        else:
            ps.append(h + 1); flip.append(0); link_d.append(0)
    return ps, flip, link_d


def links_gaf(gaf_text, node_seq_idx, seq_fwd, pos, x, y):
    return tables(observations(gaf_text, node_seq_idx, seq_fwd, pos, x, y), len(pos))


def tsv(pos, x, y, links, site_reads, node_seq_idx, min_links=MIN_LINKS):
    """the text of <out>-phase.tsv -> (text, sites, phase sets)"""
    idx = np.asarray([int(v) for v in node_seq_idx], dtype=np.int64)
    ps, flip, link_d = chain(links, min_links)
    lines = [HEADER]
    for h, p in enumerate(pos):
        node = int(np.searchsorted(idx, int(p), side="right"))
        a, b = (y[h], x[h]) if flip[h] else (x[h], y[h])
        l = [int(v) for v in links[h - link_d[h]][link_d[h] - 1]] if link_d[h] else [0, 0, 0, 0]
        f = [node, int(p) - int(idx[node - 1]), ALLELES[int(a)] + "|" + ALLELES[int(b)], ps[h], link_d[h], l[0] + l[3], l[1] + l[2]] + [int(v) for v in site_reads[h]]
        lines.append("\t".join(str(v) for v in f))
    return "\n".join(lines) + "\n", len(pos), len(set(ps))


def tsv_gaf(gaf_text, node_seq_idx, seq_fwd, min_links=MIN_LINKS, **variant_parameters):
    """the same from the alignments GAF alone -> (text, sites, phase sets, records)"""
    import variant_ref

    calls = variant_ref.call_gaf(gaf_text, node_seq_idx, seq_fwd, **variant_parameters)
    pos, x, y = sites_of(calls)
    obs = observations(gaf_text, node_seq_idx, seq_fwd, pos, x, y)
    links, sr = tables(obs, len(pos))
    text, n, sets = tsv(pos, x, y, links, sr, node_seq_idx, min_links)
    return text, n, sets, len(obs)
