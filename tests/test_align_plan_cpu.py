"""The launch plan of vga_align_batch, the parts that need no GPU: rs-vgaligner_amd/csrc/vga_align_plan.hpp compiled for the host
alone -- which (read, chain) pairs become POA problems, what the subgraph kernels are told about each, the footprint proxy and
the launch order it gives, in how many parts the subgraph store is built, and which problems count as very long, by themselves
and under VGA_SG_SPLIT / VGA_GIANT_ROWS / VGA_GIANT_CELLS.  Every expected value is the formula restated here."""
import ctypes as C
import math
import os
import random
import struct
import subprocess

import pytest

from helpers import ROOT

CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
SWITCHES = ("VGA_SUBGRAPH", "VGA_GIANT_ROWS", "VGA_GIANT_CELLS", "VGA_SG_SPLIT", "VGA_TRACE")
K = 11

HARNESS = r"""
#include "vga_align_plan.hpp"
extern "C" {
struct t_map { unsigned long long n_reads; unsigned long long *anchor_off; unsigned *qb, *tb, *te; unsigned long long *chain_off;
               unsigned char *placeholder; unsigned long long *cao; unsigned *cai; };
struct t_prob { unsigned pmin, pmax, q_first, t_first, q_last, te_last, qlen, pad, lo, hi; float west; double proxy; int reverse; };
static vga_map_result result_of(const t_map *t) {
    vga_map_result m = {};
    m.n_reads = t->n_reads; m.anchor_off = (uint64_t *)t->anchor_off; m.query_begin = t->qb; m.target_begin = t->tb; m.target_end = t->te;
    m.chain_off = (uint64_t *)t->chain_off; m.chain_placeholder = t->placeholder; m.chain_anchor_off = (uint64_t *)t->cao; m.chain_anchor_idx = t->cai;
    return m;
}
// the switches are read from the environment, as at the start of a call
unsigned long long t_select(const t_map *t, unsigned best_n, unsigned long long *prob_read, unsigned long long *prob_chain, unsigned long long *read_prob0) {
    const vga_map_result m = result_of(t);
    std::vector<uint64_t> pr, pc, p0;
    align_select(&m, best_n, pr, pc, p0);
    for (size_t i = 0; i < pr.size(); i++) { prob_read[i] = pr[i]; prob_chain[i] = pc[i]; }
    for (size_t i = 0; i < p0.size(); i++) read_prob0[i] = p0[i];
    return pr.size();
}
void t_problem(const t_map *t, unsigned long long r, unsigned long long c, unsigned qlen, unsigned k, t_prob *o) {
    const vga_map_result m = result_of(t);
    const align_prob a = align_plan_problem(&m, r, c, qlen, k, align_read_switches());
    const sg_desc &d = a.desc;
    *o = {d.pmin, d.pmax, d.q_first, d.t_first, d.q_last, d.te_last, d.qlen, d.pad, a.lo, a.hi, a.west, a.proxy, a.reverse ? 1 : 0};
}
void t_order(const double *proxy, unsigned n, unsigned *ord, unsigned *slot_of, double *permuted) {
    std::vector<double> p(proxy, proxy + n);
    const std::vector<uint32_t> o = align_launch_order(p), s = align_slot_of(o);
    align_permute(p, o);
    for (unsigned i = 0; i < n; i++) { ord[i] = o[i]; slot_of[i] = s[i]; permuted[i] = p[i]; }
}
unsigned long long t_split(const float *west, unsigned long long n, double *mean) {
    return align_store_split(std::vector<float>(west, west + n), align_read_switches(), mean);
}
int t_is_giant(unsigned N, unsigned longest, unsigned qlen, int wb, double wf) { return align_is_giant(N, longest, qlen, wb, wf, align_read_switches()); }
int t_sg_host() { return align_read_switches().sg_host; }
}
"""

U64P, U32P, U8P = C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint), C.POINTER(C.c_ubyte)


class TMap(C.Structure):
    _fields_ = [("n_reads", C.c_ulonglong), ("anchor_off", U64P), ("qb", U32P), ("tb", U32P), ("te", U32P), ("chain_off", U64P),
                ("placeholder", U8P), ("cao", U64P), ("cai", U32P)]


class TProb(C.Structure):
    _fields_ = [(n, C.c_uint) for n in ("pmin", "pmax", "q_first", "t_first", "q_last", "te_last", "qlen", "pad", "lo", "hi")] + \
               [("west", C.c_float), ("proxy", C.c_double), ("reverse", C.c_int)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("align_plan")
    src, so = d / "harness.cpp", d / "harness.so"
    src.write_text(HARNESS)
    # (a host compiler alone: the header names no HIP type and calls no HIP function)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)])
    L = C.CDLL(str(so))
    L.t_select.restype, L.t_select.argtypes = C.c_ulonglong, [C.POINTER(TMap), C.c_uint, U64P, U64P, U64P]
    L.t_problem.restype, L.t_problem.argtypes = None, [C.POINTER(TMap), C.c_ulonglong, C.c_ulonglong, C.c_uint, C.c_uint, C.POINTER(TProb)]
    L.t_order.restype, L.t_order.argtypes = None, [C.POINTER(C.c_double), C.c_uint, U32P, U32P, C.POINTER(C.c_double)]
    L.t_split.restype, L.t_split.argtypes = C.c_ulonglong, [C.POINTER(C.c_float), C.c_ulonglong, C.POINTER(C.c_double)]
    L.t_is_giant.restype, L.t_is_giant.argtypes = C.c_int, [C.c_uint, C.c_uint, C.c_uint, C.c_int, C.c_double]
    L.t_sg_host.restype = C.c_int
    return L


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)


# ------------------------------------------------------------------------------------------------ a synthetic map result
class Chains:
    """What vga_map_batch hands to vga_align_batch, as Python lists (the layout of vga_map_result)."""

    def __init__(self):
        self.qlen, self.anchor_off, self.qb, self.tb, self.te = [], [0], [], [], []
        self.chain_off, self.placeholder, self.cao, self.cai = [0], [], [0], []

    def add_read(self, qlen, anchors, chains):
        """anchors: (query_begin, target_begin, target_end); chains: lists of ascending anchor indices, [] for a placeholder"""
        self.qlen.append(qlen)
        for q, b, e in anchors:
            self.qb.append(q); self.tb.append(b); self.te.append(e)
        self.anchor_off.append(len(self.qb))
        for ch in chains:
            self.placeholder.append(0 if ch else 1)
            self.cai.extend(ch)
            self.cao.append(len(self.cai))
        self.chain_off.append(len(self.placeholder))

    def as_c(self):
        arr = lambda t, v: (t * max(1, len(v)))(*v)
        keep = [arr(C.c_ulonglong, self.anchor_off), arr(C.c_uint, self.qb), arr(C.c_uint, self.tb), arr(C.c_uint, self.te),
                arr(C.c_ulonglong, self.chain_off), arr(C.c_ubyte, self.placeholder), arr(C.c_ulonglong, self.cao), arr(C.c_uint, self.cai)]
        t = TMap(len(self.qlen), *[C.cast(a, f[1]) for a, f in zip(keep, TMap._fields_[1:])])
        t._keep = keep
        return t


def _chain_of(rng, anchors, length):
    return sorted(rng.sample(range(len(anchors)), length))


def synthetic(seed=20261016):
    """40 reads: chains of 1 to ~50 anchors, reads with only a placeholder, reads with more chains than any align_best_n used
    below, two reads with identical chains (equal proxies), one chain that spans more than 0.85 x 24 000 graph bases"""
    rng = random.Random(seed)
    m = Chains()
    for r in range(40):
        qlen = rng.randrange(800, 12000)
        if r % 9 == 4:
            m.add_read(qlen, [], [[]])   # no anchor, one placeholder
            continue
        n_anchors = rng.randrange(1, 120)
        t0 = rng.randrange(0, 3000000)
        anchors = []
        for _ in range(n_anchors):
            q = rng.randrange(0, max(1, qlen - K))
            b = t0 + q + rng.randrange(0, 400)
            anchors.append((q, b, b + K))
        anchors.sort(key=lambda a: a[2])
        n_chains = (1, 2, 3, 7, 9)[r % 5]
        chains = [_chain_of(rng, anchors, rng.randrange(1, min(50, n_anchors) + 1)) for _ in range(n_chains)]
        if r % 7 == 3:
            chains[rng.randrange(len(chains))] = []   # a placeholder among the first chains
        m.add_read(qlen, anchors, chains)
    twin = [(10, 5000, 5000 + K), (400, 5400, 5400 + K), (900, 5950, 5950 + K)]
    m.add_read(1500, twin, [[0, 1, 2]])
    m.add_read(1500, twin, [[0, 1, 2], [1]])
    m.add_read(9000, [(0, 100000, 100000 + K), (8000, 121000, 121000 + K)], [[0, 1]])   # rows > 20 400
    return m


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def py_select(m, best_n):
    prob, read_prob0 = [], []
    for r in range(len(m.qlen)):
        read_prob0.append(len(prob))
        c0, c1 = m.chain_off[r], m.chain_off[r + 1]
        for c in range(c0, c0 + min(best_n, c1 - c0)):
            if not m.placeholder[c]:
                prob.append((r, c))
    read_prob0.append(len(prob))
    return prob, read_prob0


def py_problem(m, r, c, giant_rows=24000):
    qlen, a0 = m.qlen[r], m.anchor_off[r]
    idx = [a0 + m.cai[t] for t in range(m.cao[c], m.cao[c + 1])]
    lo, hi = min(m.tb[i] for i in idx), max(m.te[i] for i in idx)
    ends = [x for i in idx for x in (m.tb[i], (m.te[i] - 1) & 0xFFFFFFFF)]
    uncovered = float(m.qb[idx[0]]) + max(0.0, float(qlen) - (float(m.qb[idx[-1]]) + float(K)))
    rows = float(hi - lo if hi > lo else 0) + 1.6 * uncovered
    west = f32(650.0 + 0.3 * max(0.0, 0.85 * rows - float(qlen)))
    proxy = rows * west + (1e13 if rows >= 0.85 * giant_rows else 0.0)
    return dict(pmin=min(ends), pmax=max(ends), q_first=m.qb[idx[0]], t_first=m.tb[idx[0]], q_last=m.qb[idx[-1]], te_last=m.te[idx[-1]],
                qlen=qlen, pad=0, lo=lo, hi=hi, west=west, proxy=proxy, reverse=int(any((m.tb[i] | m.te[i]) >> 31 for i in idx)), rows=rows)


def c_problem(lib, t, m, r, c):
    o = TProb()
    lib.t_problem(C.byref(t), r, c, m.qlen[r], K, C.byref(o))
    return o


def close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b))


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("best_n", [1, 2, 5])
def test_selection_takes_the_first_chains_of_each_read_and_skips_placeholders(lib, best_n):
    m = synthetic()
    t = m.as_c()
    cap = len(m.placeholder)
    pr, pc, p0 = (C.c_ulonglong * cap)(), (C.c_ulonglong * cap)(), (C.c_ulonglong * (len(m.qlen) + 1))()
    n = lib.t_select(C.byref(t), best_n, pr, pc, p0)
    want, want_p0 = py_select(m, best_n)
    assert [(pr[i], pc[i]) for i in range(n)] == want
    assert list(p0) == want_p0
    # what the synthetic result is meant to hold
    per_read = [want_p0[r + 1] - want_p0[r] for r in range(len(m.qlen))]
    assert 0 in per_read and max(per_read) == min(best_n, 9)
    if best_n == 5:
        assert any(m.chain_off[r + 1] - m.chain_off[r] > 5 for r in range(len(m.qlen)))
        assert any(x < min(5, m.chain_off[r + 1] - m.chain_off[r]) and x > 0 for r, x in enumerate(per_read))   # a skipped placeholder


def test_descriptor_extremes_and_proxy_of_every_problem(lib):
    m = synthetic()
    t = m.as_c()
    prob, _ = py_select(m, 9)
    lengths = set()
    bumped = 0
    for r, c in prob:
        got, want = c_problem(lib, t, m, r, c), py_problem(m, r, c)
        lengths.add(m.cao[c + 1] - m.cao[c])
        for f in ("pmin", "pmax", "q_first", "t_first", "q_last", "te_last", "qlen", "pad", "lo", "hi", "reverse"):
            assert getattr(got, f) == want[f], (r, c, f)
        assert got.reverse == 0
        assert close(got.west, want["west"]) and close(got.proxy, want["proxy"]), (r, c, got.west, want["west"], got.proxy, want["proxy"])
        assert got.west >= 650.0
        bumped += want["proxy"] >= 1e13
    assert min(lengths) == 1 and max(lengths) >= 40
    assert bumped == 1   # the chain that spans 21 000 graph bases


def test_a_long_span_goes_to_the_front_of_the_order_at_85_percent_of_the_row_threshold(lib, monkeypatch):
    def one(span):
        m = Chains()
        m.add_read(2 * K, [(0, 1000, 1000 + K), (K, 1000 + span - K, 1000 + span)], [[0, 1]])   # the chain covers the read: rows == span
        return m, m.as_c()
    for rows, env in ((24000, None), (1000, "1000"), (40000, "40000")):
        if env:
            monkeypatch.setenv("VGA_GIANT_ROWS", env)
        edge = math.ceil(0.85 * rows)
        for span, bump in ((edge - 1, 0.0), (edge, 1e13)):
            m, t = one(span)
            want = py_problem(m, 0, 0, giant_rows=rows)
            assert want["rows"] == float(span) and (want["proxy"] >= 1e13) == (bump > 0)
            assert close(c_problem(lib, t, m, 0, 0).proxy, want["proxy"])


def test_reverse_strand_anchors_are_flagged(lib):
    for where in ("begin", "end", None):
        m = Chains()
        anchors = [(0, 500, 500 + K), (100, 640, 640 + K), (300, 800, 800 + K)]
        if where == "begin":
            anchors[1] = (100, 640 | 1 << 31, 640 + K)
        if where == "end":
            anchors[2] = (300, 800, (800 + K) | 1 << 31)
        m.add_read(1000, anchors, [[0, 1, 2], [0]])
        t = m.as_c()
        assert c_problem(lib, t, m, 0, 0).reverse == (1 if where else 0)
        assert c_problem(lib, t, m, 0, 1).reverse == 0   # the chain without that anchor


def test_launch_order_is_stable_and_descending_and_slot_of_is_its_inverse(lib):
    m = synthetic()
    t = m.as_c()
    prob, _ = py_select(m, 5)
    proxies = [c_problem(lib, t, m, r, c).proxy for r, c in prob]
    assert len(set(proxies)) < len(proxies)   # the twin reads
    rng = random.Random(7)
    for proxy in (proxies, [3.0, 1.0, 3.0, 2.0, 1.0, 3.0, 0.0, 2.0], [rng.choice((1.0, 5.0, 9.0)) for _ in range(500)], [4.0], []):
        n = len(proxy)
        ord_, slot, perm = (C.c_uint * max(1, n))(), (C.c_uint * max(1, n))(), (C.c_double * max(1, n))()
        lib.t_order((C.c_double * max(1, n))(*proxy), n, ord_, slot, perm)
        want = sorted(range(n), key=lambda i: -proxy[i])   # (Python's sort is stable)
        assert list(ord_)[:n] == want
        assert all(slot[want[i]] == i for i in range(n))
        assert list(perm)[:n] == [proxy[i] for i in want]


def _split(lib, west):
    mean = C.c_double()
    return lib.t_split((C.c_float * max(1, len(west)))(*west), len(west), C.byref(mean)), mean.value


def test_store_is_split_only_for_large_calls_of_wide_problems(lib, monkeypatch):
    assert _split(lib, []) == (0, 0.0)
    for n in (1, 100, 3072):
        assert _split(lib, [2000.0] * n)[0] == n
    for n in (3073, 5000):
        assert _split(lib, [2000.0] * n)[0] == 2048
        assert _split(lib, [650.0] * n)[0] == n
        assert _split(lib, [900.0] * n)[0] == n          # mean width term <= 900: one part
        assert _split(lib, [f32(900.5)] * n)[0] == 2048   # > 900: two
        assert _split(lib, [900.0] * (n - 1) + [3000.0])[0] == 2048
    rng = random.Random(3)
    west = [f32(rng.uniform(650.0, 3000.0)) for _ in range(4000)]
    split, mean = _split(lib, west)
    want_mean = sum(west) / len(west)
    assert close(mean, want_mean) and split == 2048
    n = 5000
    for env, want in (("0", n), ("-3", n), ("100", 100), ("4999", 4999), ("5000", n), ("1000000", n)):
        monkeypatch.setenv("VGA_SG_SPLIT", env)
        assert _split(lib, [2000.0] * n)[0] == want, env
        assert _split(lib, [650.0] * n)[0] == want, env
    monkeypatch.setenv("VGA_SG_SPLIT", "100")
    assert _split(lib, [2000.0] * 50)[0] == 50


def py_is_giant(N, longest, qlen, wb, wf, giant_rows=24000, giant_cells=1.5e8):
    if N >= giant_rows:
        return 1
    ql = float(qlen)
    w = ql if wb < 0 else float(wb) + float(math.floor(wf * ql))
    ew = min(ql + 1.0, 2.0 * w + 431.0 + 0.3 * abs(float(longest) - ql))
    return 1 if N * ew >= giant_cells else 0


def _cells_edge(cells, qlen, longest, wb, wf):
    """the two row counts on either side of rows x expected width == cells"""
    ql = float(qlen)
    w = ql if wb < 0 else float(wb) + float(math.floor(wf * ql))
    ew = min(ql + 1.0, 2.0 * w + 431.0 + 0.3 * abs(float(longest) - ql))
    hi = math.ceil(cells / ew)
    while (hi - 1) * ew >= cells:
        hi -= 1
    while hi * ew < cells:
        hi += 1
    return hi - 1, hi


def test_very_long_problems_by_rows_and_by_cells(lib, monkeypatch):
    # rows alone (a short query: the cell count stays far below its threshold)
    for wb, wf in ((-1, 0.01), (10, 0.01)):
        assert lib.t_is_giant(23999, 23999, 100, wb, wf) == 0 == py_is_giant(23999, 23999, 100, wb, wf)
        assert lib.t_is_giant(24000, 24000, 100, wb, wf) == 1 == py_is_giant(24000, 24000, 100, wb, wf)
    # rows x expected width, banding off: the width is the whole query (+ 1)
    lo, hi = _cells_edge(1.5e8, 9999, 12000, -1, 0.01)
    assert (lo, hi) == (14999, 15000)
    assert lib.t_is_giant(lo, 12000, 9999, -1, 0.01) == 0 == py_is_giant(lo, 12000, 9999, -1, 0.01)
    assert lib.t_is_giant(hi, 12000, 9999, -1, 0.01) == 1 == py_is_giant(hi, 12000, 9999, -1, 0.01)
    # ... adaptive band (wb = 10, wf = 0.01): 2 w + 431 + 0.3 |longest - qlen|, here 220 + 431 + 6 000
    lo, hi = _cells_edge(1.5e8, 10000, 30000, 10, 0.01)
    assert hi < 24000 and hi * 6651.0 >= 1.5e8 > lo * 6651.0
    assert lib.t_is_giant(lo, 30000, 10000, 10, 0.01) == 0 == py_is_giant(lo, 30000, 10000, 10, 0.01)
    assert lib.t_is_giant(hi, 30000, 10000, 10, 0.01) == 1 == py_is_giant(hi, 30000, 10000, 10, 0.01)
    # a path as long as the query keeps the band narrow: the same rows are an ordinary problem
    assert lib.t_is_giant(hi, 10000, 10000, 10, 0.01) == 0 == py_is_giant(hi, 10000, 10000, 10, 0.01)
    # the switches move both thresholds
    monkeypatch.setenv("VGA_GIANT_ROWS", "1000")
    for wb in (-1, 10):
        assert lib.t_is_giant(999, 999, 100, wb, 0.01) == 0 == py_is_giant(999, 999, 100, wb, 0.01, giant_rows=1000)
        assert lib.t_is_giant(1000, 1000, 100, wb, 0.01) == 1 == py_is_giant(1000, 1000, 100, wb, 0.01, giant_rows=1000)
    monkeypatch.setenv("VGA_GIANT_ROWS", "50000")
    assert lib.t_is_giant(24000, 24000, 100, 10, 0.01) == 0 and lib.t_is_giant(49999, 49999, 100, 10, 0.01) == 0
    assert lib.t_is_giant(50000, 50000, 100, 10, 0.01) == 1
    monkeypatch.delenv("VGA_GIANT_ROWS")
    monkeypatch.setenv("VGA_GIANT_CELLS", "1e6")
    for wb, longest, qlen in ((-1, 3000, 2499), (10, 8000, 2500)):
        lo, hi = _cells_edge(1e6, qlen, longest, wb, 0.01)
        assert 0 < lo and hi < 24000
        assert lib.t_is_giant(lo, longest, qlen, wb, 0.01) == 0 == py_is_giant(lo, longest, qlen, wb, 0.01, giant_cells=1e6)
        assert lib.t_is_giant(hi, longest, qlen, wb, 0.01) == 1 == py_is_giant(hi, longest, qlen, wb, 0.01, giant_cells=1e6)
    # random sweep against the restated rule
    rng = random.Random(11)
    monkeypatch.delenv("VGA_GIANT_CELLS")
    seen = set()
    for _ in range(5000):
        N, qlen = rng.randrange(1, 40000), rng.randrange(50, 30000)
        longest, wb, wf = rng.randrange(1, 60000), rng.choice((-1, 10, 100)), rng.choice((0.01, 0.05))
        want = py_is_giant(N, longest, qlen, wb, wf)
        seen.add((want, N >= 24000))
        assert lib.t_is_giant(N, longest, qlen, wb, wf) == want, (N, longest, qlen, wb, wf)
    assert seen == {(0, False), (1, False), (1, True)}


def test_subgraph_route_switch(lib, monkeypatch):
    assert lib.t_sg_host() == 0
    monkeypatch.setenv("VGA_SUBGRAPH", "host")
    assert lib.t_sg_host() == 1
    monkeypatch.setenv("VGA_SUBGRAPH", "device")
    assert lib.t_sg_host() == 0
