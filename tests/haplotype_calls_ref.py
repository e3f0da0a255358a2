"""Reference for the haplotype counts and calls: what vga_haplotype_counts / vga_haplotype_counts_lists / vga_haplotype_jobs /
vga_haplotype_call return and what <out>-haplotype-calls.tsv holds, from what each read shows at the calls (shows_lists: from
stored lists; shows_gaf: from the text of an alignments GAF, walked as tests/pileup_ref.py walks it), the tags of
tests/haplotag_ref.py (rows / hap) and the ps of the phase chain, and from nothing else.  Written from the definition in
include/vga_hip.h with Python integers; it shares no code with the product (test infrastructure).

Columns: 0 .. 3 A C G T, 4 another letter, 5 the base is deleted, 6 the read inserts behind the base.  A read shows column k at
base p when a sparse word (p, k) names it or, for k the base's own letter (cref: 0 .. 3, 4 for anything else), when a run covers p;
once per column and base, however often the read consumes the base.  tag(r, S) is a for votes_a > votes_b of the haplotag row
(r, S), b for votes_b > votes_a, nothing otherwise.  A job (c, S) for every call with first[S] <= cpos[c] <= last[S], the smallest
and largest pos of the sites of S; by c, then by ps.  Row (c, S): c, ps, a[0 .. 6], b[0 .. 6], the reads tagged a (b) in S that show
the column at cpos[c].  Haploid call of seven counts: obs = n[0] + .. + n[5]; "." for obs = 0, else the first maximum of A C G T D,
which must hold 2 n > obs (else "?"), and "+" behind it when 2 n[6] > obs."""
import re

import numpy as np

import haplotag_ref
import phase_ref
import pileup_ref

HEADER = "node\toffset\tref\tps\ta\tb\ta_obs\tb_obs\ta_A\ta_C\ta_G\ta_T\ta_N\ta_del\ta_ins\tb_A\tb_C\tb_G\tb_T\tb_N\tb_del\tb_ins"
DEL, INS = 5, 6
_CS = re.compile(r"(:[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+)")


def cref_of(seq_fwd, cpos):
    seq = seq_fwd.decode() if isinstance(seq_fwd, (bytes, bytearray)) else str(seq_fwd)
    return [pileup_ref.column(seq[int(p)]) for p in cpos]


def shows_lists(recs, words, cpos, cref):
    """-> shows[n_reads]: {call index: set of columns}"""
    call_at = {int(p): c for c, p in enumerate(cpos)}
    out = []
    for off, n_runs, n_sparse in [[int(v) for v in r] for r in recs]:
        seen = {}
        ev = [int(w) for w in words[off:off + n_runs]]
        for i in range(0, n_runs, 2):
            for p in range(ev[i] >> 1, ev[i + 1] >> 1):
                if p in call_at:
                    seen.setdefault(call_at[p], set()).add(min(4, int(cref[call_at[p]])))
        for w in [int(w) for w in words[off + n_runs:off + n_runs + n_sparse]]:
            if (w >> 3) in call_at:
                seen.setdefault(call_at[w >> 3], set()).add(w & 7)
        out.append(seen)
    return out


def shows_gaf(gaf_text, node_seq_idx, seq_fwd, cpos):
    """the same from the aligned records of the text, in order: ":N" shows the own letter of each base it covers, "*gq" shows q,
    "-g.." shows "deleted" at each of its bases, "+q.." shows "inserts" at the base consumed most recently before it (nothing when
    no base was consumed yet)"""
    idx = [int(v) for v in node_seq_idx]
    seq = seq_fwd.decode() if isinstance(seq_fwd, (bytes, bytearray)) else str(seq_fwd)
    call_at = {int(p): c for c, p in enumerate(cpos)}
    out = []
    for line in gaf_text.splitlines():
        f = line.split("\t")
        if len(f) < 12 or f[5] == "*":
            continue
        path = [int(v) for v in f[5][1:].split(">")]
        toks = _CS.findall(re.search(r"cs:Z:([^,\s]*)", "\t".join(f[11:])).group(1))
        seen, pi, off, last = {}, 0, int(f[7]), None
        for t in toks:
            if t[0] == "+":
                if last in call_at:
                    seen.setdefault(call_at[last], set()).add(INS)
                continue
            items = [None] * int(t[1:]) if t[0] == ":" else [pileup_ref.column(t[2])] if t[0] == "*" else [DEL] * (len(t) - 1)
            for col in items:
                while off == idx[path[pi]] - idx[path[pi] - 1]:
                    pi, off = pi + 1, 0
                p = idx[path[pi] - 1] + off
                if p in call_at:
                    seen.setdefault(call_at[p], set()).add(pileup_ref.column(seq[p]) if col is None else col)
                last = p
                off += 1
        assert pi == len(path) - 1 and off == int(f[8]), "the walk must end at path_end on the last node"
        out.append(seen)
    return out


def tags(obs, ps, flip):
    """-> {(read, ps): "a" or "b"} from the rows of the haplotag reference"""
    return {(r, p): haplotag_ref.hap(a, b) for r, p, a, b in haplotag_ref.rows(obs, ps, flip) if a != b}


def jobs(cpos, pos, ps):
    """-> [(c, ps)] by c, then by ps"""
    first, last = {}, {}
    for h, p in enumerate(pos):
        s = int(ps[h])
        first[s] = min(first.get(s, int(p)), int(p))
        last[s] = max(last.get(s, int(p)), int(p))
    return [(c, s) for c, p in enumerate(cpos) for s in sorted(first) if first[s] <= int(p) <= last[s]]


def counts(shows, tag, job_list):
    """-> rows [[c, ps, a0 .. a6, b0 .. b6]]"""
    out = []
    for c, s in job_list:
        row = [c, s] + [0] * 14
        for r, seen in enumerate(shows):
            t = tag.get((r, s))
            if t is not None:
                for k in seen.get(c, ()):
                    row[2 + k + (7 if t == "b" else 0)] += 1
        out.append(row)
    return out


def table(shows, obs, cpos, pos, ps, flip):
    """the same as the uint32 array the library returns"""
    return np.array(counts(shows, tags(obs, ps, flip), jobs(cpos, pos, ps)), dtype=np.uint32).reshape(-1, 16)


def call(n):
    n = [int(v) for v in n]
    assert len(n) == 7
    obs = sum(n[:6])
    if obs == 0:
        return "."
    of = [n[0], n[1], n[2], n[3], n[5]]
    best = of.index(max(of))  # the first maximum
    return ("ACGT-"[best] if 2 * of[best] > obs else "?") + ("+" if 2 * n[6] > obs else "")


def tsv(rows, cpos, node_seq_idx, seq_fwd):
    """the text of <out>-haplotype-calls.tsv -> (text, jobs, lines, lines whose two decided calls differ)"""
    idx = np.asarray([int(v) for v in node_seq_idx], dtype=np.int64)
    seq = seq_fwd.decode() if isinstance(seq_fwd, (bytes, bytearray)) else str(seq_fwd)
    lines, differ = [HEADER], 0
    for row in rows:
        row = [int(v) for v in row]
        a, b = row[2:9], row[9:16]
        if sum(a) + sum(b) == 0:
            continue
        p = int(cpos[row[0]])
        node = int(np.searchsorted(idx, p, side="right"))
        ca, cb = call(a), call(b)
        differ += ca[0] not in ".?" and cb[0] not in ".?" and ca != cb
        lines.append("\t".join(str(v) for v in [node, p - int(idx[node - 1]), seq[p], row[1], ca, cb, sum(a[:6]), sum(b[:6])] + a + b))
    return "\n".join(lines) + "\n", len(rows), len(lines) - 1, differ


def gaf(gaf_text, node_seq_idx, seq_fwd, min_links=phase_ref.MIN_LINKS, **variant_parameters):
    """everything from the alignments GAF alone -> dict(calls, cpos, pos, x, y, ps, flip, obs, shows, rows)"""
    import variant_ref

    calls = variant_ref.call_gaf(gaf_text, node_seq_idx, seq_fwd, **variant_parameters)
    cpos = [int(p) for p in calls["pos"]]
    pos, x, y = phase_ref.sites_of(calls)
    obs = phase_ref.observations(gaf_text, node_seq_idx, seq_fwd, pos, x, y)
    ps, flip, _ = phase_ref.chain(phase_ref.tables(obs, len(pos))[0], min_links)
    shows = shows_gaf(gaf_text, node_seq_idx, seq_fwd, cpos)
    assert len(shows) == len(obs)
    return {"calls": calls, "cpos": cpos, "pos": pos, "x": x, "y": y, "ps": ps, "flip": flip, "obs": obs, "shows": shows,
            "rows": counts(shows, tags(obs, ps, flip), jobs(cpos, pos, ps))}


def tsv_gaf(gaf_text, node_seq_idx, seq_fwd, min_links=phase_ref.MIN_LINKS, **variant_parameters):
    g = gaf(gaf_text, node_seq_idx, seq_fwd, min_links, **variant_parameters)
    return tsv(g["rows"], g["cpos"], node_seq_idx, seq_fwd)
