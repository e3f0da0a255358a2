"""Synthetic cases for the haplotype counts (vga_haplotype_counts_lists, the seam): a case of tests/phase_cases.py plus the calls
(cpos ascending, cref the own letter of each: 0 .. 3 A C G T, 4 anything else), the sets (ps, flip) and, for the cases written out by
hand, the jobs and the rows."""
import collections

import numpy as np

import phase_cases as P

A, C, G, T, D = range(5)
COL_OTHER, COL_DEL, COL_INS = 4, 5, 6

HapCase = collections.namedtuple("HapCase", "name n_bases pos x y ref reads cpos cref ps flip")


def phase_case(h):
    return P.Case(h.name, h.n_bases, h.pos, h.x, h.y, h.ref, h.reads)


# ---- by hand: four A / C sites whose own letter is A, in two interleaved sets (set 1: sites 0 and 2, bases 5 .. 20, site 2 flipped;
# set 2: sites 1 and 3, bases 10 .. 30) and nine calls: one before every site (2), one behind every site (35), one in set 1 alone (5,
# 7), three in both (10, 15, 20), two in set 2 alone (25, 30).  The own letters of the calls: A A G A N A T A C.
HAND = HapCase("hand", 40, [5, 10, 20, 30], [A] * 4, [C] * 4, [A] * 4, [
    ([(0, 40)], []),                                              # 0: A everywhere.  set 1: a at site 0, b at the flipped site 2: tied; set 2: a
    ([(0, 20), (21, 40)], [(20, C)]),                             # 1: C at the flipped site: a, a in set 1; a in set 2
    ([], [(5, C), (10, C), (20, A), (7, COL_DEL), (15, COL_INS), (25, COL_OTHER), (7, G)]),   # 2: b in set 1 (2 : 0), b in set 2 (site 1 alone)
    ([(6, 9)], [(7, T), (15, C)]),                                # 3: consumes no site: no tag anywhere
    ([(5, 6), (14, 16)], [(15, COL_INS), (15, COL_INS), (2, A), (35, A)]),   # 4: a in set 1 (site 0 alone), no vote in set 2
], [2, 5, 7, 10, 15, 20, 25, 30, 35], [A, A, G, A, COL_OTHER, A, T, A, C], [1, 2, 1, 2], [0, 0, 1, 0])
HAND_JOBS = [(1, 1), (2, 1), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (5, 2), (6, 2), (7, 2)]
# tags: set 1: read 1 a, read 2 b, read 4 a (read 0 tied, read 3 none); set 2: reads 0 and 1 a, read 2 b
HAND_ROWS = [
    #  c ps  a: A  C  G  T  N  D  I   b: A  C  G  T  N  D  I
    [1, 1, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],   # base 5: reads 1 and 4 run over it (A); read 2 shows C
    [2, 1, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0],   # base 7 (G): read 1's run; read 2 shows deleted and G; the tied read 0 and read 3 count nowhere
    [3, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],   # base 10 in set 1: read 1 (A); read 2 (C); read 4 does not reach it
    [3, 2, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0],   # base 10 in set 2: reads 0 and 1
    [4, 1, 0, 0, 0, 0, 2, 0, 1, 0, 0, 0, 0, 0, 0, 1],   # base 15 (N): runs of reads 1 and 4 show "other"; read 4 inserts (twice: once); read 2 inserts
    [4, 2, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 1],   # in set 2 reads 0 and 1 are a, read 4 has no tag
    [5, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0],   # base 20: read 1 shows C, read 2 A
    [5, 2, 1, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0],   # in set 2 read 0 (A) counts too
    [6, 2, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0],   # base 25 (T): reads 0 and 1; read 2 shows another letter
    [7, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # base 30: reads 0 and 1; read 2 does not reach it
]


def columns_case(copies=1):
    """one set of two A / C sites (bases 10 and 20); calls at bases 12 .. 18, call k for column k, and their own letters A C G T N A
    A.  Four kinds of reads -- tagged a, tagged b, tied, no row -- and each shows column k at call k by a sparse word; then the same
    four kinds with a run over bases 12 .. 18 (the own letters: columns 0 .. 4, and A twice more) and one word, T, at call 0 beside
    the run: two columns at one base.  -> (case, rows)"""
    kinds = [[(10, A), (20, A)], [(10, C), (20, C)], [(10, A), (20, C)], []]
    words = [(12 + k, k) for k in range(7)]
    reads = ([([], kind + words) for kind in kinds] + [([(12, 19)], kind + [(12, T)]) for kind in kinds]) * copies
    case = HapCase("columns", 30, [10, 20], [A, A], [C, C], [A, A], reads, list(range(12, 19)), [A, C, G, T, COL_OTHER, A, A], [1, 1], [0, 0])
    rows = []
    for c in range(7):
        n = [0] * 7
        n[c] += 1                                     # the sparse word of the first kind of read
        n[[A, C, G, T, COL_OTHER, A, A][c]] += 1      # the run of the second
        if c == 0:
            n[T] += 1                                 # and its word
        rows.append([c, 1] + [copies * v for v in n] * 2)
    return case, rows


def with_calls(case, n_calls, ps, flip, seed):
    """a case of phase_cases with n_calls calls: about half of them on sites (their own letter is the site's), the others anywhere;
    always the first and the last base when there is room, so that some calls lie outside every set"""
    rng = np.random.default_rng(seed)
    on = [int(p) for p in rng.choice(case.pos, size=min(len(case.pos), n_calls // 2), replace=False)] if case.pos else []
    free = [p for p in range(case.n_bases) if p not in set(on)]
    want = [p for p in (0, case.n_bases - 1) if p in free][:max(0, n_calls - len(on))]
    rest = [p for p in free if p not in want]
    more = [int(p) for p in rng.choice(rest, size=n_calls - len(on) - len(want), replace=False)]
    cpos = sorted(on + want + more)
    assert len(cpos) == n_calls == len(set(cpos))
    site = {int(p): h for h, p in enumerate(case.pos)}
    cref = [int(case.ref[site[p]]) if p in site else int(rng.integers(0, 5)) for p in cpos]
    return HapCase(case.name, case.n_bases, case.pos, case.x, case.y, case.ref, case.reads, cpos, cref, list(ps), [int(v) for v in flip])
