"""Synthetic read generator for the BASELINE.json workloads (host-side tooling, numpy only).

The reference simulates reads with `vg sim -s 77` (experiments-snakemake/Snakefile:32), which is not
available offline.  This module samples reads from the GFA's own P lines instead:
  * a path is drawn uniformly among the paths stored on the forward strand (the mapper only keeps
    forward/forward anchors, src/map.rs:62; a path written with '-' steps is skipped),
  * the start offset is uniform in [0, len(path) - read_len],
  * errors are i.i.d. per template base: substitution / insertion / deletion with the given rates,
    indel lengths geometric(p=0.7) (see _mutate for the exact rule),
  * PRNG: numpy PCG64 seeded with 77.
Config #2: 150 bp, 1 % substitutions.  Config #3: 10 kbp, 3 % sub / 3 % ins / 4 % del ("ONT-like").
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Tuple

import numpy as np


def parse_gfa_paths(gfa_path: str) -> Tuple[Dict[int, str], List[Tuple[str, List[Tuple[int, bool]]]]]:
    segs: Dict[int, str] = {}
    paths: List[Tuple[str, List[Tuple[int, bool]]]] = []
    with open(gfa_path) as f:
        for ln in f:
            if ln.startswith("S\t"):
                p = ln.rstrip("\n").split("\t")
                segs[int(p[1])] = p[2]
            elif ln.startswith("P\t"):
                p = ln.rstrip("\n").split("\t")
                steps = [(int(s[:-1]), s[-1] == "-") for s in p[2].split(",") if s]
                paths.append((p[1], steps))
    return segs, paths


_COMP = str.maketrans("ACGTNacgtn", "TGCANtgcan")


def path_sequence(segs: Dict[int, str], steps: List[Tuple[int, bool]]) -> str:
    out = []
    for nid, rev in steps:
        s = segs[nid]
        out.append(s[::-1].translate(_COMP) if rev else s)
    return "".join(out)


@dataclass
class SimRead:
    name: str
    seq: str
    path: str
    offset: int
    template_len: int = 0  # bases of the source path the read was drawn from (before errors)
    strand: str = "+"      # "-": seq is the reverse complement of the read drawn from the path


_SWITCH = {ord(a): b for a, b in zip("ACGTUacgtu", "TGCAAtgcaa")}


def reverse_complement(s: str) -> str:
    """the reference's switch_base over the reversed read (src/dna.rs:20-33): any byte outside it becomes N"""
    return "".join(_SWITCH.get(ord(c), "N") for c in reversed(s))


def _mutate(tpl: np.ndarray, rng: np.random.Generator, sub: float, ins: float, dele: float) -> bytes:
    """Vectorised error model.  Every template base draws one category:
    substitution (a different base), insertion (geometric(0.7) random bases BEFORE the base, the base
    itself kept), deletion start (this base and the following geometric(0.7)-1 bases are dropped), or
    copy.  Events on a base that an earlier deletion removed are dropped with it."""
    L = tpl.shape[0]
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    u = rng.random(L)
    is_sub = u < sub
    is_ins = (u >= sub) & (u < sub + ins)
    is_del = (u >= sub + ins) & (u < sub + ins + dele)
    out = tpl.copy()
    ns = int(is_sub.sum())
    if ns:
        # a different base: rotate the 2-bit code by 1..3
        code = np.searchsorted(bases, out[is_sub])
        code = np.where(bases[np.clip(code, 0, 3)] == out[is_sub], code, 0)
        out[is_sub] = bases[(code + rng.integers(1, 4, size=ns)) & 3]
    keep = np.ones(L, dtype=bool)
    nd = int(is_del.sum())
    if nd:
        starts = np.flatnonzero(is_del)
        lens = rng.geometric(0.7, size=nd)
        diff = np.zeros(L + 1, dtype=np.int32)
        np.add.at(diff, starts, 1)
        np.add.at(diff, np.minimum(starts + lens, L), -1)
        keep = np.cumsum(diff[:L]) == 0
    reps = np.ones(L, dtype=np.int64)
    ni = int(is_ins.sum())
    if ni:
        reps[is_ins] += rng.geometric(0.7, size=ni)
    reps[~keep] = 0
    res = np.repeat(out, reps)
    if ni:
        # positions of inserted bases: all but the last copy of each repeated run of an insertion site
        ends = np.cumsum(reps)
        site = np.flatnonzero(is_ins & keep)
        if site.size:
            mask = np.zeros(res.shape[0], dtype=bool)
            for e, n in zip(ends[site], reps[site]):
                mask[e - n:e - 1] = True
            res[mask] = bases[rng.integers(0, 4, size=int(mask.sum()))]
    return res.tobytes()


def simulate_reads(gfa_path: str, n_reads: int, read_len: int, sub: float, ins: float, dele: float,
                   seed: int = 77, forward_only: bool = True, reverse_fraction: float = 0.0) -> List[SimRead]:
    """reverse_fraction: the share of reads that come out as the reverse complement of what was drawn (strand "-").  The coin
    comes from a generator of its own, so the draws of the forward reads -- and every read set made without it -- are unchanged."""
    segs, paths = parse_gfa_paths(gfa_path)
    seqs = []
    for name, steps in paths:
        if forward_only and any(rev for _, rev in steps):
            continue
        seqs.append((name, np.frombuffer(path_sequence(segs, steps).encode(), dtype=np.uint8)))
    if not seqs:
        raise ValueError("no forward path in " + gfa_path)
    rng = np.random.Generator(np.random.PCG64(seed))
    coin = np.random.Generator(np.random.PCG64([seed, 0x5eed])).random(n_reads) if reverse_fraction > 0 else None
    reads: List[SimRead] = []
    for r in range(n_reads):
        pi = int(rng.integers(0, len(seqs)))
        name, ps = seqs[pi]
        L = min(read_len, ps.shape[0])
        off = int(rng.integers(0, ps.shape[0] - L + 1))
        tpl = ps[off:off + L]
        if sub == 0 and ins == 0 and dele == 0:
            seq = tpl.tobytes().decode()
        else:
            seq = _mutate(tpl, rng, sub, ins, dele).decode()
        if coin is not None and coin[r] < reverse_fraction:
            reads.append(SimRead(f"read{r}", reverse_complement(seq), name, off, L, "-"))
        else:
            reads.append(SimRead(f"read{r}", seq, name, off, L))
    return reads


def config2_reads(gfa_path: str, n_reads: int = 1000) -> List[SimRead]:
    return simulate_reads(gfa_path, n_reads, 150, 0.01, 0.0, 0.0, seed=77)


def config3_reads(gfa_path: str, n_reads: int = 10000, read_len: int = 10000) -> List[SimRead]:
    return simulate_reads(gfa_path, n_reads, read_len, 0.03, 0.03, 0.04, seed=77)


def truth_gaf(gfa_path: str, reads: List[SimRead]) -> str:
    """The GAF a perfect aligner would write for simulated reads, as far as the node path goes: one record per read
    whose path field lists the nodes the read's template [offset, offset + template length) overlaps on its source
    path (what `vg sim -a` + `vg convert --gam-to-gaf` provide in the reference's experiments, Snakefile:32-40).
    The template length is not stored; it is bounded by the read's own source window: reads are cut from the path
    at `offset` with the requested length before errors are applied, so the window is recomputed from the path."""
    segs, paths = parse_gfa_paths(gfa_path)
    by_name = {name: steps for name, steps in paths}
    out = []
    for r in reads:
        steps = by_name[r.path]
        lens = [len(segs[n]) for n, _ in steps]
        total = sum(lens)
        tpl = min(getattr(r, "template_len", 0) or len(r.seq), total - r.offset)
        lo, hi = r.offset, r.offset + tpl
        pos, nodes = 0, []
        for (nid, rev), ln in zip(steps, lens):
            if pos < hi and pos + ln > lo:
                nodes.append(("<" if rev else ">") + str(nid))
            pos += ln
            if pos >= hi:
                break
        out.append("\t".join([r.name, str(len(r.seq)), "0", str(len(r.seq)), getattr(r, "strand", "+"), "".join(nodes), str(tpl), "0", str(tpl), "0",
                              str(tpl), "255", "ta:Z:truth"]))
    return "\n".join(out) + ("\n" if out else "")


def write_fasta(reads: List[SimRead], path: str) -> None:
    """single-line FASTA: the reference emits one read per sequence line (src/io.rs:100-122)"""
    with open(path, "w") as f:
        for r in reads:
            f.write(f">{r.name}\n{r.seq}\n")


# ---------------------------------------------------------------------------------------------------------
# graphs of BASELINE.json configs #4 and #5

# The 20 HLA-zoo loci of the reference's experiments (experiments-snakemake/*/graph.gfa, kept as data under
# tests/golden/data).  The reference requires `odgi sort`-ed input (README.md:24-28) and odgi is not available offline; only
# nine loci are forward-only, acyclic and topologically numbered as shipped (HLA_FORWARD_ACYCLIC).  toposort_gfa below is
# the stand-in for `odgi sort` that makes the other eleven usable: config #4 = the disjoint union of all 20, sorted.
HLA_FORWARD_ACYCLIC = ["hla/1-simple", "DRB1-3123", "hla/6-DRB5-3127", "hla/11-C-3107-spoa", "hla/12-DMA-3108-spoa",
                       "hla/13-V-352962-spoa", "hla/14-DOB-3112-spoa", "hla/18-B-3106-smooth", "hla/19-MICB-4227-smooth"]
HLA_ALL = ["hla/1-simple", "DRB1-3123", "hla/3-E3133", "hla/4-A3105", "hla/5-B3106", "hla/6-DRB5-3127", "hla/7-MICB-4277", "hla/8-C3107",
           "hla/9-G-3135", "hla/10-F-3134", "hla/11-C-3107-spoa", "hla/12-DMA-3108-spoa", "hla/13-V-352962-spoa", "hla/14-DOB-3112-spoa",
           "hla/15-H-3136-spoa", "hla/16-DQB1-3119-spoa", "hla/17-DRB1-3123-smooth", "hla/18-B-3106-smooth", "hla/19-MICB-4227-smooth",
           "hla/20-C3107-smooth"]
# Config #4 takes 19 of the 20: 7-MICB-4277 stays cyclic after sorting (10 self loops, 94 back edges among 1-2 bp nodes) and
# the reference's k-mer enumeration (src/kmer.rs:347-505 with its default max_furcations = 100) does not finish on it -- in
# the reference no more than here, whose index builder restates it -- so the locus is left out, by name.  Three more keep
# a few back edges (5-B3106: 22, 8-C3107: 31, 16-DQB1-3119-spoa: 7, 10-F-3134 / 15-H-3136-spoa: 1), which the POA subgraph
# drops by the reference's own src < dst rule; 17-DRB1-3123-smooth (15 links) and 20-C3107-smooth (2) are not
# strand-consistent, so every path of theirs has reverse steps and the forward-only mapper gets no reads from them.
HLA_CONFIG4 = [n for n in HLA_ALL if n != "hla/7-MICB-4277"]


def toposort_gfa(in_path: str, out_path: str) -> Dict[str, int]:
    """Stand-in for `odgi sort` (README.md:24-28 of the reference): re-orient and re-number a GFA so that ids follow a
    topological order of the forward links.
      1. strand: nodes are flipped (sequence reverse-complemented, link and path orientations toggled) so that as many links
         as possible join equal orientations -- a 2-colouring of the link graph, breadth first from the lowest id, links in
         file order, and of the two colourings the one in which the paths mostly run forward; a link that still joins opposite orientations afterwards is kept as it is ("mixed": the component
         is not strand-consistent there);
      2. a link between two reversed handles is the same edge read from the other side: a- -> b-  becomes  b+ -> a+;
      3. order: Kahn's algorithm over the forward links (self loops and mixed links do not constrain it), always taking the
         ready node that a path visits first (then the lowest old id).  When a cycle leaves no ready node, the remaining
         node that a path visits first is taken: its unresolved in-links become back edges (to_id <= from_id), which the
         reference's POA subgraph drops by its own rule (src/align.rs:717-721) -- a cyclic locus stays usable, and the
         counts say how cyclic it is;
      4. ids 1..n in that order; S lines in id order, L lines in file order, P lines re-oriented.
    Returns counts: nodes, links, bases, flipped, mixed_links, self_loops, back_edges, cycle_breaks."""
    import heapq

    S: Dict[int, str] = {}
    L: List[Tuple[int, bool, int, bool, str]] = []
    P: List[Tuple[str, List[Tuple[int, bool]]]] = []
    header = "H\tVN:Z:1.0"
    with open(in_path) as f:
        for ln in f:
            p = ln.rstrip("\n").split("\t")
            if p[0] == "S":
                S[int(p[1])] = p[2]
            elif p[0] == "L":
                L.append((int(p[1]), p[2] == "-", int(p[3]), p[4] == "-", p[5] if len(p) > 5 else "0M"))
            elif p[0] == "P":
                P.append((p[1], [(int(x[:-1]), x[-1] == "-") for x in p[2].split(",") if x]))
            elif p[0] == "H":
                header = ln.rstrip("\n")
    adj: Dict[int, List[Tuple[int, bool]]] = {n: [] for n in S}
    for a, ra, b, rb, _ in L:
        adj[a].append((b, ra != rb))
        adj[b].append((a, ra != rb))
    flip: Dict[int, bool] = {}
    steps_of: Dict[int, List[int]] = {n: [0, 0] for n in S}  # per node: path steps written forward / reverse
    for _, steps in P:
        for nid, rev in steps:
            steps_of[nid][1 if rev else 0] += 1
    for s0 in sorted(S):
        if s0 in flip:
            continue
        flip[s0] = False
        queue, qi = [s0], 0
        while qi < len(queue):
            u = queue[qi]
            qi += 1
            for v, x in adj[u]:
                if v not in flip:
                    flip[v] = flip[u] ^ x
                    queue.append(v)
        # of the two consistent orientations of the component, the one in which the paths mostly run forward
        fwd = sum(steps_of[u][1 if flip[u] else 0] for u in queue)
        rev = sum(steps_of[u][0 if flip[u] else 1] for u in queue)
        if rev > fwd:
            for u in queue:
                flip[u] = not flip[u]
    links = []  # (from, from_rev, to, to_rev, overlap) after flips, reversed pairs turned around
    n_mixed = n_self = 0
    for a, ra, b, rb, ov in L:
        ra, rb = ra ^ flip[a], rb ^ flip[b]
        if ra and rb:
            a, b, ra, rb = b, a, False, False
        if ra != rb:
            n_mixed += 1
        elif a == b:
            n_self += 1
        links.append((a, ra, b, rb, ov))
    first_visit: Dict[int, int] = {}
    t = 0
    for _, steps in P:
        for nid, _ in steps:
            if nid not in first_visit:
                first_visit[nid] = t
            t += 1
    key = lambda n: (first_visit.get(n, 1 << 60), n)
    indeg = {n: 0 for n in S}
    out: Dict[int, List[int]] = {n: [] for n in S}
    for a, ra, b, rb, _ in links:
        if not ra and not rb and a != b:
            indeg[b] += 1
            out[a].append(b)
    ready = [key(n) for n in S if indeg[n] == 0]
    heapq.heapify(ready)
    rest = sorted((key(n) for n in S if indeg[n] > 0))
    rest_i = 0
    done = set()
    order: List[int] = []
    n_breaks = 0
    while len(order) < len(S):
        if ready:
            _, u = heapq.heappop(ready)
            if u in done:
                continue
        else:  # a cycle: take the remaining node a path reaches first
            while rest[rest_i][1] in done:
                rest_i += 1
            u = rest[rest_i][1]
            n_breaks += 1
        done.add(u)
        order.append(u)
        for v in out[u]:
            indeg[v] -= 1
            if indeg[v] == 0 and v not in done:
                heapq.heappush(ready, key(v))
    new_id = {old: i + 1 for i, old in enumerate(order)}
    n_back = 0
    with open(out_path, "w") as f:
        f.write(header + "\n")
        for old in order:
            seq = S[old]
            f.write("S\t%d\t%s\n" % (new_id[old], seq[::-1].translate(_COMP) if flip[old] else seq))
        for a, ra, b, rb, ov in links:
            if not ra and not rb and new_id[b] <= new_id[a]:
                n_back += 1
            f.write("L\t%d\t%s\t%d\t%s\t%s\n" % (new_id[a], "-" if ra else "+", new_id[b], "-" if rb else "+", ov))
        for name, steps in P:
            f.write("P\t%s\t%s\t*\n" % (name, ",".join("%d%s" % (new_id[n], "-" if (r ^ flip[n]) else "+") for n, r in steps)))
    return {"nodes": len(S), "links": len(L), "bases": sum(len(x) for x in S.values()), "flipped": sum(1 for x in flip.values() if x),
            "mixed_links": n_mixed, "self_loops": n_self, "back_edges": n_back, "cycle_breaks": n_breaks}


def config4_graph(data_dir: str, out_path: str, loci: List[str] = None) -> Tuple[int, int, int]:
    """the merged HLA graph of config #4 ("all HLA-zoo loci merged"): every locus of HLA_CONFIG4 through toposort_gfa, then
    their disjoint union.  Returns (nodes, edges, bases) = (23980, 33177, 282231); (24754, 34369, 298386) for all 20."""
    import os
    import tempfile

    loci = HLA_CONFIG4 if loci is None else loci
    with tempfile.TemporaryDirectory() as td:
        parts = []
        for i, n in enumerate(loci):
            sp = os.path.join(td, "%02d.gfa" % i)
            toposort_gfa(os.path.join(data_dir, n + ".gfa"), sp)
            parts.append(sp)
        return merge_gfas(parts, out_path)


def merge_gfas(gfa_paths: List[str], out_path: str) -> Tuple[int, int, int]:
    """Disjoint union of GFA graphs with cumulative id offsets (ids stay contiguous and topological when every input's
    are).  Path names get the input's ordinal as a prefix.  Returns (nodes, edges, bases)."""
    off = 0
    n_edges = n_bases = 0
    with open(out_path, "w") as out:
        out.write("H\tVN:Z:1.0\n")
        for gi, gp in enumerate(gfa_paths):
            top = 0
            with open(gp) as f:
                for ln in f:
                    p = ln.rstrip("\n").split("\t")
                    if p[0] == "S":
                        top = max(top, int(p[1]))
                        n_bases += len(p[2])
                        out.write("S\t%d\t%s\n" % (int(p[1]) + off, p[2]))
                    elif p[0] == "L":
                        n_edges += 1
                        out.write("L\t%d\t%s\t%d\t%s\t%s\n" % (int(p[1]) + off, p[2], int(p[3]) + off, p[4], p[5] if len(p) > 5 else "0M"))
                    elif p[0] == "P":
                        steps = ",".join("%d%s" % (int(s[:-1]) + off, s[-1]) for s in p[2].split(",") if s)
                        out.write("P\tg%d_%s\t%s\t*\n" % (gi, p[1], steps))
            off += top
    return off, n_edges, n_bases


def synth_pangenome(out_path: str, total_bp: int = 1_000_000, seed: int = 77, n_haps: int = 16, mean_node: int = 32,
                    snp_every: int = 100, indel_every: int = 1000) -> Tuple[int, int, int]:
    """Config #5: a random backbone (uniform ACGT) cut into nodes of mean `mean_node` bp (geometric), a SNP bubble
    about every `snp_every` bp and a 1-20 bp indel bubble about every `indel_every` bp; ids are assigned in
    topological order (what `odgi sort -p Ygs` would produce); `n_haps` haplotype paths pick bubble arms at random.
    Returns (nodes, edges, bases)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    segs: List[bytes] = []
    edges: List[Tuple[int, int]] = []
    # per backbone step: ("n", id) plain node, ("s", ref, alt) SNP arms, ("i", id) optional indel node
    plan: List[Tuple] = []
    made = 0
    p_snp = mean_node / snp_every
    p_indel = mean_node / indel_every

    def new_node(n):
        segs.append(acgt[rng.integers(0, 4, size=n)].tobytes())
        return len(segs)  # 1-based id

    prev: List[int] = []
    skip_from: List[int] = []  # nodes that may also jump over the next (optional) node
    while made < total_bp:
        n = int(rng.geometric(1.0 / mean_node))
        a = new_node(n)
        made += n
        for pnode in prev + skip_from:
            edges.append((pnode, a))
        plan.append(("n", a))
        prev, skip_from = [a], []
        u = rng.random()
        if made >= total_bp:
            break
        if u < p_snp:
            ref = new_node(1)
            b = int(rng.integers(1, 4))
            alt_base = acgt[(int(np.searchsorted(acgt, segs[ref - 1][0])) + b) & 3]
            segs.append(bytes([alt_base]))
            alt = len(segs)
            edges += [(a, ref), (a, alt)]
            plan.append(("s", ref, alt))
            prev = [ref, alt]
            made += 1
        elif u < p_snp + p_indel:
            ins = new_node(int(rng.integers(1, 21)))
            edges.append((a, ins))
            plan.append(("i", ins))
            prev, skip_from = [ins], [a]
            made += len(segs[ins - 1])
    with open(out_path, "w") as out:
        out.write("H\tVN:Z:1.0\n")
        for i, s in enumerate(segs):
            out.write("S\t%d\t%s\n" % (i + 1, s.decode()))
        for a, b in sorted(edges):
            out.write("L\t%d\t+\t%d\t+\t0M\n" % (a, b))
        for h in range(n_haps):
            steps = []
            for st in plan:
                if st[0] == "n":
                    steps.append(st[1])
                elif st[0] == "s":
                    steps.append(st[1] if rng.random() < 0.5 else st[2])
                elif rng.random() < 0.5:
                    steps.append(st[1])
            out.write("P\thap%d\t%s\t*\n" % (h, ",".join("%d+" % s for s in steps)))
    return len(segs), len(edges), sum(len(s) for s in segs)
