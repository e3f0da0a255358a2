"""The genotype measure in plain numpy, from its definition (include/vga_hip.h) and from nothing in the library: for two
n_reads x n_paths matrices and every pair p <= q, the per-read lexicographic maximum of (bases, edges) summed by component, and how
many reads prefer either side; and the ranking of the pairs."""
import numpy as np

FIELDS = ("sum_bases", "sum_edges", "prefer_a", "prefer_b")


def pair_index(n_paths, p, q):
    return p * n_paths - p * (p - 1) // 2 + (q - p)


def pairs(bases, edges):
    """-> {sum_bases, sum_edges, prefer_a, prefer_b: uint64[P (P + 1) / 2] in row-major upper-triangle order, n_paths}"""
    b = np.asarray(bases, dtype=np.uint64)
    e = np.asarray(edges, dtype=np.uint64)
    assert b.ndim == 2 and b.shape == e.shape
    n_paths = b.shape[1]
    p, q = np.triu_indices(n_paths)
    out = {k: np.zeros(len(p), dtype=np.uint64) for k in FIELDS}
    for r in range(b.shape[0]):  # a row at a time: P (P + 1) / 2 values each
        bp, bq, ep, eq = b[r, p], b[r, q], e[r, p], e[r, q]
        q_wins = (bq > bp) | ((bq == bp) & (eq > ep))
        p_wins = (bp > bq) | ((bp == bq) & (ep > eq))
        out["sum_bases"] += np.where(q_wins, bq, bp)
        out["sum_edges"] += np.where(q_wins, eq, ep)
        out["prefer_a"] += p_wins.astype(np.uint64)
        out["prefer_b"] += q_wins.astype(np.uint64)
    out["n_paths"] = n_paths
    return out


def add(x, y):
    assert x["n_paths"] == y["n_paths"]
    out = {k: x[k] + y[k] for k in FIELDS}
    out["n_paths"] = x["n_paths"]
    return out


def rank(table, top=None):
    """the pairs (p, q) whose sums are not (0, 0), best first: sum_bases, then sum_edges, both descending, then the homozygous pair,
    then p, then q"""
    n = table["n_paths"]
    rows = []
    i = 0
    for p in range(n):
        for q in range(p, n):
            sb, se = int(table["sum_bases"][i]), int(table["sum_edges"][i])
            if sb or se:
                rows.append((-sb, -se, 0 if p == q else 1, p, q))
            i += 1
    rows.sort()
    return [(p, q) for _, _, _, p, q in rows][:top if top else None]


def same(got, want, what=""):
    assert got["n_paths"] == want["n_paths"], what
    for k in FIELDS:
        g, w = got[k], want[k]
        assert g.dtype == np.uint64 and g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, k, len(bad), bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())
