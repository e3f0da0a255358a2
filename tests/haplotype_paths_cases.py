"""Synthetic cases for the haplotype paths through the kernel seam (vga_haplotype_paths_lists): the stored lists of
tests/phase_cases.py with a row of deficit bytes and a scored byte per read, at the smallest shapes where k_hp_sums can still go wrong,
and for the smallest cases the groups written out by hand."""
import collections

import numpy as np

import phase_cases as P

HpCase = collections.namedtuple("HpCase", "name case ps flip deficits scored")

# n_paths around the pitch of four bytes, a lane's four paths, a wave's word and a workgroup's chunk of 256 paths
PATH_COUNTS = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257)
READ_COUNTS = (1, 63, 64, 65, 129)
SET_COUNTS = (1, 2, 64, 65)

# ---- by hand, on P.TINY (observations P.TINY_OBS) under ps = [1, 2], flip = [0, 0]:
#   read 0: a in set 0, b in set 1;  read 1: b, b;  read 2: a, a;  read 3: no vote in set 0 (other), b in set 1 -- but unscored;
#   read 4 and read 5: no word or no site, tagged nowhere (read 4 is scored all the same)
TINY_DEFICITS = np.array([[0, 5, 9], [7, 0, 0], [0, 0, 64], [1, 2, 0], [0, 3, 3], [0, 0, 0]], dtype=np.uint8)
TINY_SCORED = np.array([1, 1, 1, 0, 1, 0], dtype=np.uint8)
TINY = HpCase("tiny", P.TINY, [1, 2], [0, 0], TINY_DEFICITS, TINY_SCORED)
TINY_READS = [2, 1, 1, 2]
TINY_COST = [[0, 5, 73], [7, 0, 0], [0, 0, 64], [7, 5, 9]]
TINY_BEST = [[2, 1, 0], [0, 1, 1], [1, 1, 0], [1, 1, 1]]
# one set with site 1 flipped: reads 1 and 2 tie, read 0 and the unscored read 3 go with a, nobody with b
TINY_ONE = HpCase("tiny, one set", P.TINY, [1, 1], [0, 1], TINY_DEFICITS, TINY_SCORED)
TINY_ONE_READS = [1, 0]
TINY_ONE_COST = [[0, 5, 9], [0, 0, 0]]
TINY_ONE_BEST = [[1, 0, 0], [0, 0, 0]]


def table_of(cost, best):
    t = np.zeros((len(cost), len(cost[0]), 2), dtype=np.uint64)
    t[:, :, 0], t[:, :, 1] = np.array(cost, dtype=np.uint64), np.array(best, dtype=np.uint64)
    return t


def random_rows(rng, n_reads, n_paths, unscored_every=7):
    """rows with a zero somewhere (the best path), zeros in runs, bytes at the top of the range, and every few reads an unscored
    one whose row is NOT zero: the sum must leave it out by the scored byte alone"""
    d = rng.integers(0, 256, size=(n_reads, n_paths), dtype=np.uint64).astype(np.uint8)
    d[rng.random((n_reads, n_paths)) < 0.3] = 0
    d[rng.random((n_reads, n_paths)) < 0.1] = 255
    for r in range(n_reads):
        d[r, int(rng.integers(0, n_paths))] = 0
    scored = np.ones(n_reads, dtype=np.uint8)
    scored[unscored_every - 1::unscored_every] = 0
    d[scored == 0] = 9
    return d, scored


def interleaved(n_sites, n_sets):
    """ps of n_sets sets whose sites interleave: site h opens set h for h < n_sets and joins set h % n_sets afterwards"""
    return [(h % n_sets) + 1 for h in range(n_sites)]


def paths_case(n_paths, n_reads=70, n_sites=8, n_sets=3, seed=0):
    case = P.random_case("paths", n_reads, n_sites, seed=9000 + 7 * n_paths + n_reads + seed)
    rng = np.random.default_rng(100 + n_paths + n_reads + seed)
    d, scored = random_rows(rng, n_reads, n_paths)
    return HpCase("%d paths, %d reads, %d sets" % (n_paths, n_reads, n_sets), case, interleaved(n_sites, min(n_sets, n_sites)),
                  [int(v) for v in rng.integers(0, 2, size=n_sites)], d, scored)


def sets_case(n_sets, n_paths=5, seed=0):
    """2 S sites: the first S open the S sets, the others join sets at random; reads that are tagged in the first, the middle and
    the last set"""
    n_sites = 2 * n_sets if n_sets > 1 else 1
    case = P.random_case("sets", 150, n_sites, seed=8000 + n_sets + seed)
    rng = np.random.default_rng(8000 + n_sets + seed)
    ps = [h + 1 for h in range(n_sets)] + [int(rng.integers(1, n_sets + 1)) for _ in range(n_sites - n_sets)]
    flip = [int(v) for v in rng.integers(0, 2, size=n_sites)]
    col = lambda a: P.COL_DEL if a == P.D else a
    reads = list(case.reads)
    for s in (0, n_sets // 2, n_sets - 1):
        reads.append(([], [(case.pos[s], col(case.x[s]))]))
        reads.append(([], [(case.pos[s], col(case.y[s]))]))
    d, scored = random_rows(rng, len(reads), n_paths, unscored_every=11)
    scored[-6:] = 1
    return HpCase("%d sets" % n_sets, case._replace(reads=reads), ps, flip, d, scored)


def kinds_case(n_reads, shift, n_paths=6):
    """four sites in two interleaved sets (own letter neither allele: a run would show "other"); read r is of kind (r + shift) % 6:
    (a, a), (a, b), (a tie in set 1, b in set 0 -- tagged in one and tied in the other), no vote at all, (b, a), and (a, a) but
    unscored.  The row of a read of kind k is k + 1 everywhere but at path k, where it is 0."""
    A, Cc = P.A, P.C
    pos = [2, 5, 8, 11]
    kinds = [([], [(2, A), (5, A)]), ([], [(2, A), (5, Cc)]), ([], [(2, A), (8, Cc), (5, Cc)]), ([], []), ([], [(2, Cc), (8, Cc), (5, A), (11, A)]),
             ([], [(2, A), (5, A)])]
    kind = [(r + shift) % 6 for r in range(n_reads)]
    d = np.array([[0 if p == k else k + 1 for p in range(n_paths)] for k in kind], dtype=np.uint8)
    scored = np.array([0 if k == 5 else 1 for k in kind], dtype=np.uint8)
    return HpCase("kinds", P.Case("kinds", 16, pos, [A] * 4, [Cc] * 4, [P.G] * 4, [kinds[k] for k in kind]), [1, 2, 1, 2], [0, 0, 0, 0], d, scored), kind


def kinds_groups(kind, n_paths=6):
    """the four groups of kinds_case by hand: set 0 (sites 0 and 2), set 1 (sites 1 and 3).  kind 0: a in both; kind 1: a in set 0,
    b in set 1; kind 2: A at site 0 and C at site 2 tie in set 0, C at site 1: b in set 1; kind 3: nowhere; kind 4: C C in set 0: b, A A
    in set 1: a; kind 5: unscored"""
    member = {0: (0, 2), 1: (0, 3), 2: (3,), 3: (), 4: (1, 2), 5: ()}
    reads = [0] * 4
    cost = [[0] * n_paths for _ in range(4)]
    best = [[0] * n_paths for _ in range(4)]
    for k in kind:
        for g in member[k]:
            reads[g] += 1
            for p in range(n_paths):
                cost[g][p] += 0 if p == k else k + 1
                best[g][p] += 1 if p == k else 0
    return np.array(reads, dtype=np.uint64), table_of(cost, best)


def wide_scores():
    """matrices for the deficit rule itself (tests/haplotype_paths_ref.py: deficits): a row of all-equal scores (every path is best),
    deficits of exactly cap - 1, cap and cap + 1 for cap 1, 64 and 255, a row whose bases + edges passes 2^32 (the sum is 64 bits),
    and a row of zeros (unscored) -> (bases, edges) uint32"""
    top = 0xFFFFFFFF
    bases = np.array([[7, 7, 7, 7, 7, 7], [300, 300 - 63, 300 - 64, 300 - 65, 299, 300 - 255], [300, 300 - 254, 300 - 256, 0, 300, 46],
                      [top, top, top - 1, 1 << 31, 0, top], [0, 0, 0, 0, 0, 0]], dtype=np.uint32)
    edges = np.array([[1, 1, 1, 1, 1, 1], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 0], [top, top - 64, top, 1 << 31, 0, 3], [0, 0, 0, 0, 0, 0]], dtype=np.uint32)
    return bases, edges


# the rows of wide_scores() under three caps, by hand
WIDE_DEFICITS = {
    1: [[0] * 6, [0, 1, 1, 1, 0, 1], [0, 1, 1, 1, 0, 1], [0, 1, 1, 1, 1, 1], [0] * 6],
    64: [[0] * 6, [0, 63, 64, 64, 0, 64], [0, 64, 64, 64, 0, 64], [0, 64, 1, 64, 64, 64], [0] * 6],
    255: [[0] * 6, [0, 63, 64, 65, 0, 255], [0, 254, 255, 255, 0, 254], [0, 64, 1, 255, 255, 255], [0] * 6],
}
WIDE_SCORED = [1, 1, 1, 1, 0]
