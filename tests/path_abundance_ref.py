"""The path abundance in plain numpy uint64 / Python integers, from its definition (include/vga_hip.h, csrc/vga_abundance.hpp): rows
of byte deficits and scored bytes, the table W, theta in units of 2^-24 from the uniform start, and per iteration
    term = theta W[d],  z = sum_p term,  resp = (term << 16) // z,  S = sum_r resp,  theta' = (S << 24) // sum_p S,
    diff = max_p |theta' - theta|
until diff <= tol (converged) or `iters` iterations; and the text `vgaligner map --path-abundance` writes.  W is an argument: the
library's table (binding.path_abundance_table), so that two platforms' exp2 cannot make the GPU and this file differ; table_float is
numpy's own evaluation, for the test that holds the library's table against it.  It shares no code with the product; from a GAF the
rows come from path_support_ref.walk or path_edit_ref.walk."""
import numpy as np

import path_edit_ref
import path_support_ref

THETA_BITS, RESP_BITS = 24, 16
HEADER = "rank\tpath\tppm\ttheta\treads_q16\tbest"


def table_float(lam, cap):
    """W[d] = max(1, floor(65536 2^(-lam d / 256) + 0.5)), d = 0..cap, in numpy's float64, then repeated to 256 entries"""
    d = np.arange(cap + 1, dtype=np.float64)
    w = np.maximum(1, np.floor(65536.0 * np.exp2(-float(lam) * d / 256.0) + 0.5)).astype(np.int64)
    return np.concatenate([w, np.full(255 - cap, w[cap], dtype=np.int64)])


def deficits(bases, edges, cap):
    """-> (d uint8[n, n_paths], scored uint8[n]): k_gl_deficit's rule"""
    assert 1 <= cap <= 255
    s = np.asarray(bases, dtype=np.uint64) + np.asarray(edges, dtype=np.uint64)
    assert s.ndim == 2
    if s.size == 0:
        return np.zeros(s.shape, dtype=np.uint8), np.zeros(s.shape[0], dtype=np.uint8)
    m = s.max(axis=1, keepdims=True)
    return np.minimum(m - s, np.uint64(cap)).astype(np.uint8), (m[:, 0] != 0).astype(np.uint8)


def ppm(theta):
    return (int(theta) * 1000000) >> THETA_BITS


def estimate(d, scored, W, iters=1000, tol=16, trace=None):
    """-> {theta uint32[n_paths], reads_q16 uint64[n_paths], best uint64[n_paths], n_scored, iterations, converged, n_paths}.
    trace: a list that receives (theta, S, diff) of every iteration.  The bounds of the definition are asserted on the way."""
    d = np.asarray(d, dtype=np.uint8)
    scored = np.asarray(scored, dtype=np.uint8).reshape(-1)
    W = np.asarray(W, dtype=np.uint64)
    assert d.ndim == 2 and d.shape[0] == len(scored) and W.shape == (256,) and scored.max(initial=0) <= 1
    assert 1 <= iters <= 100000 and 0 <= tol <= 1 << 24
    n_paths = d.shape[1]
    assert 1 <= n_paths <= 4096
    rows = d[scored != 0]
    n = len(rows)
    assert n < 1 << 23
    out = dict(theta=np.zeros(n_paths, dtype=np.uint32), reads_q16=np.zeros(n_paths, dtype=np.uint64), best=np.zeros(n_paths, dtype=np.uint64), n_scored=n,
               iterations=0, converged=False, n_paths=n_paths)
    if n == 0:
        return out
    out["best"] = np.count_nonzero(rows == 0, axis=0).astype(np.uint64)
    w = W[rows]                                                      # [n, n_paths]: at most 65536
    theta = np.full(n_paths, (1 << THETA_BITS) // n_paths, dtype=np.uint64)
    for it in range(1, iters + 1):
        term = theta[None, :] * w                                    # <= 2^40
        z = term.sum(axis=1, keepdims=True)
        assert int(term.max()) <= 1 << 40 and 1 <= int(z.min()) and int(z.max()) <= 1 << 40
        resp = (term << np.uint64(RESP_BITS)) // z                   # numerator <= 2^56
        S = resp.sum(axis=0)
        total = int(S.sum())
        assert total >= 16 * n and int(S.max()) < 1 << 40           # (S << 24 stays below 2^64)
        new = (S << np.uint64(THETA_BITS)) // np.uint64(total)
        diff = int(np.abs(new.astype(np.int64) - theta.astype(np.int64)).max())
        theta = new
        if trace is not None:
            trace.append((theta.astype(np.uint32), S.copy(), diff))
        out["iterations"] = it
        if diff <= tol:
            out["converged"] = True
            break
    out["theta"], out["reads_q16"] = theta.astype(np.uint32), S.astype(np.uint64)
    return out


def gaf_rows(gaf_text, gfa, cap, source="support", reads=None):
    """the store of a run from its alignments GAF: a row per record that is no placeholder, in GAF order -> (d, scored, path names).
    source "edit" needs `reads`, the read sequences in GAF order."""
    if source == "support":
        node_len, paths = path_support_ref.parse_gfa(gfa)
        w = path_support_ref.walk(gaf_text, node_len, paths)
        b, e = w["bases"], w["edges"]
    else:
        _, paths = path_edit_ref.parse_gfa(gfa)
        b, e = path_edit_ref.likelihood_matrices(path_edit_ref.walk(gaf_text, reads, gfa))
    lines = [ln for ln in gaf_text.splitlines() if ln]
    keep = [r for r, ln in enumerate(lines) if ln.split("\t")[5] != "*"]
    d, scored = deficits(np.asarray(b)[keep], np.asarray(e)[keep], cap)
    return d, scored, [p[0] for p in paths]


def same(got, want, what=""):
    for k in ("n_paths", "n_scored", "iterations", "converged"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k, dt in (("theta", np.uint32), ("reads_q16", np.uint64), ("best", np.uint64)):
        g, w = got[k], want[k]
        assert g.dtype == dt and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, k, len(bad), bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())


def order(theta):
    """the paths by theta descending, then in P-line order"""
    return sorted(range(len(theta)), key=lambda p: (-int(theta[p]), p))


def tsv(res, names, min_ppm=10000):
    """<out>-path-abundance.tsv: one line per path with ppm >= min_ppm, by theta descending then P-line order; the header alone
    without a call"""
    lines = [HEADER]
    if res["n_scored"]:
        rank = 0
        for p in order(res["theta"]):
            if ppm(res["theta"][p]) >= min_ppm:
                rank += 1
                lines.append("%d\t%s\t%d\t%d\t%d\t%d" % (rank, names[p], ppm(res["theta"][p]), int(res["theta"][p]), int(res["reads_q16"][p]), int(res["best"][p])))
    return "".join(ln + "\n" for ln in lines)


def stderr_line(res, n_kept, min_ppm=10000):
    if not res["n_scored"]:
        return "path-abundance: no call"
    shown = [ppm(res["theta"][p]) for p in order(res["theta"]) if ppm(res["theta"][p]) >= min_ppm]
    return "path-abundance: %d reads scored of %d kept, %d iterations (%s), %d paths at or above %d ppm%s" % (
        res["n_scored"], n_kept, res["iterations"], "converged" if res["converged"] else "not converged", len(shown), min_ppm,
        (": " + ", ".join("%d ppm" % v for v in shown)) if shown else "")
