"""Synthetic stored lists for the phase kernels (vga_phase_links_lists, the seam) and, for the smallest cases, the observations and
tables written out by hand.  A case is a graph of n_bases bases, sites (pos, x, y, ref) and reads given as (runs, sparse):
runs = [(start, end)] covers the bases start .. end - 1, sparse = [(position, column)] with the columns of a sparse word
(0 .. 3 the read shows A C G T, 4 another letter, 5 the base is deleted, 6 an insertion behind the base)."""
import collections

import numpy as np

A, C, G, T, D = range(5)
COL_OTHER, COL_DEL, COL_INS = 4, 5, 6
REF_OTHER = 4

Case = collections.namedtuple("Case", "name n_bases pos x y ref reads")


def pack(reads):
    """reads -> (recs[n, 3] uint32, words uint32): per read its run-event words in pairs, then its sparse words"""
    recs, words = [], []
    for runs, sparse in reads:
        ev = []
        for start, end in runs:
            ev += [start << 1, (end << 1) | 1]
        recs.append((len(words), len(ev), len(sparse)))
        words += ev + [(p << 3) | col for p, col in sparse]
    return np.array(recs, dtype=np.uint32).reshape(-1, 3), np.array(words, dtype=np.uint32)


# ---- the smallest case: two sites, every way a run can meet a site.  Site 0 at base 3 holds A / G and its own letter is A (x);
# site 1 at base 7 holds C / T and its own letter is T (y).
TINY = Case("tiny", 20, [3, 7], [A, C], [G, T], [A, T], [
    ([(0, 20)], []),                          # one run over everything: own letters, x at site 0 and y at site 1
    ([(0, 3), (4, 8)], [(3, G)]),             # a run that ends AT site 0 does not cover it; the mismatch shows G = y; the second run covers 7
    ([(3, 4)], [(7, C)]),                     # a run that starts at site 0 covers it; C = x at site 1
    ([(7, 8)], [(3, COL_DEL)]),               # a deleted base at a site without D: other
    ([], []),                                 # a read with no word at all
    ([(5, 7)], [(3, COL_INS)]),               # an insertion behind site 0 is no observation of it; the run ends at site 1
])
TINY_OBS = [[0, 1], [1, 1], [0, 0], [2, 1], [3, 3], [3, 3]]
# links[0][d = 1]: (x, x) read 2, (x, y) read 0, (y, x) none, (y, y) read 1
TINY_LINKS = np.zeros((2, 8, 4), dtype=np.uint32)
TINY_LINKS[0, 0] = [1, 1, 0, 1]
TINY_SITE_READS = np.array([[2, 1, 1], [1, 3, 0]], dtype=np.uint32)

# ---- edges: sites at base 0 and at the last base, a deletion allele, a site whose own letter is neither allele, one whose own
# letter is N, bases consumed twice
EDGE = Case("edge", 40, [0, 10, 11, 20, 39], [A, C, A, G, A], [C, D, G, T, T], [A, C, T, REF_OTHER, T], [
    ([(0, 40)], []),                                                     # spans every site
    ([(0, 10), (11, 12)], [(10, COL_DEL)]),                              # ends at site 1 (not covered), D = y there
    ([(1, 11)], [(11, A), (20, COL_OTHER), (39, COL_INS)]),              # ends one behind site 1 (covered); N is other; ins ignored
    ([(11, 12), (20, 21)], [(0, A), (0, C), (10, C), (10, C), (11, G), (20, T), (39, T), (39, A)]),  # every site consumed twice
    ([], []),
    ([(0, 1), (39, 40)], [(20, G)]),                                     # runs of one base at the first and at the last base
])
EDGE_OBS = [[0, 0, 2, 2, 1],
            [0, 1, 2, 3, 3],
            [3, 0, 0, 2, 3],
            [2, 0, 1, 1, 2],   # x then y: 2; x twice: 0; own letter (other) and y: 1, twice; y then x: 2
            [3, 3, 3, 3, 3],
            [0, 3, 3, 0, 1]]


def far_case():
    """ten sites; reads that see site 0 and site 8 (eight apart: linked) and reads that see site 0 and site 9 (nine apart: not
    linked at all), and nothing in between"""
    pos = [5 * h + 2 for h in range(10)]
    reads = [([], [(pos[0], A), (pos[8], A)])] * 3 + [([], [(pos[0], C), (pos[8], A)])] * 2 + [([], [(pos[0], A), (pos[9], C)])] * 4
    return Case("far", 60, pos, [A] * 10, [C] * 10, [G] * 10, reads)


def random_case(name, n_reads, n_sites, seed, n_bases=None):
    """reads of random runs and sparse words over random sites, on them and beside them"""
    rng = np.random.default_rng(seed)
    n_bases = n_bases or 7 * n_sites + 9
    pos = sorted(int(p) for p in rng.choice(np.arange(0, n_bases), size=n_sites, replace=False))
    x = [int(v) for v in rng.integers(0, 4, size=n_sites)]
    y = [int(rng.integers(a + 1, 5)) for a in x]
    ref = [int(rng.choice([x[h], y[h] if y[h] < 4 else x[h], rng.integers(0, 5)])) for h in range(n_sites)]   # mostly one of the alleles
    col_of = lambda a: COL_DEL if a == D else a
    at = {p: h for h, p in enumerate(pos)}
    reads = []
    for _ in range(n_reads):
        runs, sparse, p = [], [], int(rng.integers(0, n_bases))
        end = min(n_bases, p + int(rng.integers(1, 12 * 7)))
        while p < end:
            kind = int(rng.integers(0, 10))
            if kind < 6:
                q = min(end, p + int(rng.integers(1, 15)))
                runs.append((p, q))
                p = q
            elif kind < 9:
                h = at.get(p)   # at a site: mostly one of its alleles
                sparse.append((p, int(rng.integers(0, 6)) if h is None or rng.integers(0, 4) == 0 else col_of([x[h], y[h]][int(rng.integers(0, 2))])))
                p += 1
            else:
                sparse.append((max(0, p - 1), COL_INS))
                p += int(rng.integers(0, 3))
        if rng.integers(0, 8) == 0 and n_sites:  # a base consumed once more
            sparse.append((pos[int(rng.integers(0, n_sites))], int(rng.integers(0, 6))))
        reads.append((runs, sparse))
    return Case(name, n_bases, pos, x, y, ref, reads)


def planted_sample(readsim, gfa, node_seq_idx, seed=11, n_reads=12, length=1000):
    """Two haplotypes from one path of DRB1 (the template and the node of test_planted_substitution_is_reported: the first node of
    50 bases or more behind offset 2000 of path 3).  Three substitutions no path has, at a quarter, a half and three quarters of
    the node: haplotype A carries the first and the third, haplotype B the second.  n_reads reads per haplotype with 1 % of each
    error, tiled so that every read covers the three sites.
    -> (reads [(name, sequence)], graph bases of the three sites, planted letters, letters of the path)"""
    idx = [int(v) for v in node_seq_idx]
    segs, paths = readsim.parse_gfa_paths(gfa)
    _, steps = paths[3]
    assert not any(rev for _, rev in steps)
    off = 0
    for nid, _ in steps:
        if off >= 2000 and len(segs[nid]) >= 50:
            break
        off += len(segs[nid])
    ln = len(segs[nid])
    offs = [ln // 4, ln // 2, 3 * ln // 4]
    at_path, at_graph = [off + o for o in offs], [idx[nid - 1] + o for o in offs]
    seq = readsim.path_sequence(segs, steps)
    old = [seq[p].upper() for p in at_path]
    new = ["ACGT"[("ACGT".index(c) + 1) % 4] for c in old]
    hap_a, hap_b = list(seq), list(seq)
    hap_a[at_path[0]], hap_a[at_path[2]], hap_b[at_path[1]] = new[0], new[2], new[1]
    rng = np.random.Generator(np.random.PCG64(seed))
    reads, span = [], at_path[2] - at_path[0]
    for name, hap in (("a", "".join(hap_a)), ("b", "".join(hap_b))):
        for r in range(n_reads):
            o = at_path[2] - length + 1 + (r + 1) * (length - span - 1) // (n_reads + 1)
            assert o <= at_path[0] and o + length > at_path[2]
            tpl = np.frombuffer(hap[o:o + length].encode(), dtype=np.uint8)
            reads.append(("%s%d" % (name, r), readsim._mutate(tpl, rng, 0.01, 0.01, 0.01).decode()))
    return reads, at_graph, new, old
