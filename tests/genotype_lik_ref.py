"""The diploid read likelihood of every pair of paths in plain numpy, from its definition (include/vga_hip.h): for two
n_reads x n_paths matrices, s = bases + edges in 64 bits, d = min(row maximum of s - s, cap), and for every pair p <= q the sum over the
rows of lam min(d_p, d_q) + T[|d_p - d_q|]; and the ranking of the pairs.  T is an argument: the library's table
(binding.genotype_likelihood_table), so that two platforms' log2 cannot make the GPU and this file differ.  table_float is numpy's own
evaluation of T, for the test that holds the library's table against it."""
import numpy as np


def pair_index(n_paths, p, q):
    return p * n_paths - p * (p - 1) // 2 + (q - p)


def table_float(lam, cap):
    """T[x] = round(256 (1 - log2(1 + 2^(-lam x / 256)))), x = 0..cap, in numpy's float64"""
    x = np.arange(cap + 1, dtype=np.float64)
    return np.floor(256.0 * (1.0 - np.log2(1.0 + np.exp2(-float(lam) * x / 256.0))) + 0.5).astype(np.int64)


def deficits(bases, edges, cap):
    """-> (d: uint8[n_reads, n_paths], n_scored)"""
    s = np.asarray(bases, dtype=np.uint64) + np.asarray(edges, dtype=np.uint64)
    assert s.ndim == 2
    if s.shape[0] == 0 or s.shape[1] == 0:
        return np.zeros(s.shape, dtype=np.uint8), 0
    m = s.max(axis=1, keepdims=True)
    return np.minimum(m - s, np.uint64(cap)).astype(np.uint8), int(np.count_nonzero(m))


def pairs(bases, edges, lam, cap, T):
    """-> {cost: uint64[P (P + 1) / 2] in row-major upper-triangle order, deficit, n_scored, n_paths}"""
    T = np.asarray(T, dtype=np.uint64)
    assert T.shape == (cap + 1,)
    d, n_scored = deficits(bases, edges, cap)
    n_paths = d.shape[1]
    p, q = np.triu_indices(n_paths)
    cost = np.zeros(len(p), dtype=np.uint64)
    d64 = d.astype(np.int64)
    for r in range(d.shape[0]):  # a row at a time: P (P + 1) / 2 values each
        dp, dq = d64[r, p], d64[r, q]
        cost += np.uint64(lam) * np.minimum(dp, dq).astype(np.uint64) + T[np.abs(dp - dq)]
    return {"cost": cost, "deficit": d, "n_scored": n_scored, "n_paths": n_paths}


def add(x, y):
    assert x["n_paths"] == y["n_paths"]
    return {"cost": x["cost"] + y["cost"], "n_scored": x["n_scored"] + y["n_scored"], "n_paths": x["n_paths"]}


def rank(cost, n_paths, top=None):
    """[(p, q, cost, margin)] from the cheapest up: cost, then the homozygous pair, then p, then q; margin over the first"""
    rows = []
    i = 0
    for p in range(n_paths):
        for q in range(p, n_paths):
            rows.append((int(cost[i]), 0 if p == q else 1, p, q))
            i += 1
    rows.sort()
    first = rows[0][0] if rows else 0
    return [(p, q, c, c - first) for c, _, p, q in rows][:top if top else None]


def same(got, want, what="", deficit=True):
    assert got["n_paths"] == want["n_paths"], what
    assert got["n_scored"] == want["n_scored"], (what, got["n_scored"], want["n_scored"])
    if deficit:
        g, w = got["deficit"], want["deficit"]
        assert g.dtype == np.uint8 and g.shape == w.shape, (what, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, "deficit", len(bad), bad[:6].tolist())
    g, w = got["cost"], want["cost"]
    assert g.dtype == np.uint64 and g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero(g != w)
    assert len(bad) == 0, (what, "cost", len(bad), bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())
