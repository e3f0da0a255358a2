"""Seeded POA problems that plant the COLUMN axis of the DP kernels: where a row's band starts and ends relative to a lane's 4 or
8 columns, a wave, a step of 4 NT / 8 NT columns and the LDS window -- what `_rand_problem` and the read simulators leave to
chance.  Plain Python: no GPU, no oracle.  A problem is `(nodes, edges, query)` as in tests/poa_topologies.py; `params` holds the
vga_poa_params fields that differ from the defaults (problems of equal params can share one vga_poa_batch call: `groups`).

With a half-width w and a read that is an exact path of a linear graph the band of row r is [r - w, r + w] (clipped to the
query): the row phase beg % 8 sweeps every value and end - (beg - beg % 8) = 2 w + phase, so one unit of w moves a problem
across each threshold below and the rows of one problem alternate between its two sides.

The second half of the file restates, row by row, the branch each kernel takes from the band (beg, end) of every row -- the
oracle's OG_POA_ROWS (oracle_py.poa_align_rows) or the library's VGA_POA_DUMP_ROWS.  tests/test_poa_band_cases_cpu.py holds
`fixed_set()` to the branches it is there for; tests/test_poa_band_cases_gpu.py runs it and counts hand-backs with
`t6_hands_back` / `t7_hands_back`."""
import random
from collections import namedtuple

from poa_topologies import RING_SPAN, _seq

T4_CPL = 4          # columns per lane of k_poa_dp_t4 / _t5 / _lds<NT, 4> (vga_poa_t5.hpp:62: STEP = NT * 4)
T6_CPL = 8          # columns per lane of k_poa_dp_t6 / _t7 (vga_poa_t6.hpp:143: nbase = beg / CPL * CPL; vga_poa_t7.hpp:154: beg & ~7)
T6_WIN = 64 * T6_CPL  # k_poa_dp_t6's window (vga_poa_t6.hpp:48): a second step from end - nbase >= WIN (:145), handed back from 2 WIN (:144)
T6_RING_SLOT = (6 * (2 * T6_WIN + 8) + 15) & ~15  # vga_poa_t6.hpp:93: its value-row ring has fixed slots of 6 192 bytes
WIDE_PAD = 8        # k_poa_dp_t4 / _t5: a row is wide when W + 8 > window (vga_poa_t5.hpp:354)
T7_PAD = 9          # k_poa_dp_t7 hands back when end - nbase + 1 + 8 > window (vga_poa_t7.hpp:155)

SLIDE_W = tuple(range(120, 129)) + tuple(range(248, 259)) + tuple(range(502, 515))
FLAT_QLEN = (247, 248, 251, 252, 503, 504, 507, 508, 511, 512, 513, 1015, 1016, 1019, 1020, 1023, 1024, 1025, 2047, 2048, 2049)
JUMP_INS = (7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 600)
JUMP_DEL = (23, 24, 25, 63, 64, 65, 200)
JUMP_AT = 600
JUMP_BANDS = (("default", {}), ("w200", {"wb": 200, "wf": 0.0}), ("w253", {"wb": 253, "wf": 0.0}))
NCOL_W = (60, 253)
NCOL_COLS = (0, 3, 4, 7, 8, 255, 256, 257, 511, 512, 513, -1)  # column j stands for query[j - 1]: column 0 is taken as the first base, -1 is the last
BUBBLE_W = (253, 509)
LEAD = ((259, 250, 1000), (560, 462, 1036))  # (graph bases deleted, w, at base)
LINE_NODE, LINE_LEN = 40, 1600

Case = namedtuple("Case", "name family problem params")


def line(rng, n=LINE_LEN, node=LINE_NODE):
    """a linear graph of n random bases in nodes of `node` bases: (nodes, edges)"""
    s = _seq(rng, n)
    nodes = [s[i:i + node] for i in range(0, n, node)]
    return nodes, [(v, v + 1) for v in range(len(nodes) - 1)]


def banded(w):
    return {"wb": w, "wf": 0.0}


def slide_cases(seed=11):
    nodes, edges = line(random.Random(seed))
    q = "".join(nodes)
    return [Case(f"slide-w{w}", "slide", (nodes, edges, q), banded(w)) for w in SLIDE_W]


def flat_problem(rng, qlen, g=40):
    """a two-node line of g bases that occurs in the middle of a random query of qlen bases"""
    s = _seq(rng, g)
    nodes, edges = [s[:g // 2], s[g // 2:]], [(0, 1)]
    head = (qlen - g) // 2
    return nodes, edges, _seq(rng, head) + s + _seq(rng, qlen - g - head)


def flat_cases(seed=12):
    return [Case(f"flat-q{n}", "flat", flat_problem(random.Random(seed * 10000 + n), n), {"wb": -1}) for n in FLAT_QLEN]


def jump_queries(rng, nodes, at=JUMP_AT, ins=JUMP_INS, dels=JUMP_DEL):
    s = "".join(nodes)
    return [(f"ins{n}", s[:at] + _seq(rng, n) + s[at:]) for n in ins] + [(f"del{n}", s[:at] + s[at + n:]) for n in dels]


def jump_cases(seed=13):
    rng = random.Random(seed)
    nodes, edges = line(rng)
    reads = jump_queries(rng, nodes)
    return [Case(f"jump-{tag}-{band}", "jump", (nodes, edges, q), dict(kw)) for band, kw in JUMP_BANDS for tag, q in reads]


def ncol_cases(seed=14):
    nodes, edges = line(random.Random(seed))
    s = "".join(nodes)
    at = sorted({(len(s) if c < 0 else max(c, 1)) - 1 for c in NCOL_COLS})
    out = []
    for w in NCOL_W:
        for c in NCOL_COLS:
            i = (len(s) if c < 0 else max(c, 1)) - 1
            out.append(Case(f"ncol-w{w}-c{'last' if c < 0 else c}", "ncol", (nodes, edges, s[:i] + "N" + s[i + 1:]), banded(w)))
        q = "".join("N" if i in at else ch for i, ch in enumerate(s))
        out.append(Case(f"ncol-w{w}-all", "ncol", (nodes, edges, q), banded(w)))
    return out


def bubble_graph(rng, n_bubbles=14, seg=(99, 100, 101, 102)):
    """A SNP (two one-base alleles) about every 100 bases: the stretches between them cycle through the lengths of `seg`, so
    that the rows behind a bubble fall on every phase of the band's first column.  Returns (nodes, edges, second alleles)"""
    nodes, edges, second = [_seq(rng, seg[0])], [], []
    for k in range(n_bubbles):
        a = rng.choice("ACGT")
        b = rng.choice([x for x in "ACGT" if x != a])
        s = len(nodes) - 1
        nodes += [a, b, _seq(rng, seg[(k + 1) % len(seg)])]
        edges += [(s, s + 1), (s, s + 2), (s + 1, s + 3), (s + 2, s + 3)]
        second.append(s + 2)
    return nodes, edges, second


def bubble_cases(seed=15):
    nodes, edges, second = bubble_graph(random.Random(seed))
    q = "".join(s for v, s in enumerate(nodes) if len(s) > 1 or v in second)
    return [Case(f"bubble-w{w}", "bubble", (nodes, edges, q), banded(w)) for w in BUBBLE_W]


def lead_cases(seed=17):
    """`slide`'s line with D graph bases missing from the read at base `at`, under a band of D + w just below a step of 512 and of
    1 024 columns.  Above the deletion the diagonal of the band runs D columns left of the read's path, so the band is
    [r - D - w, r + w] and the path lies D + w columns right of its first column: with the row phase the matched cells of the
    optimal path fall on the last column of a step and on the first of the next one (in `slide` the path is w columns from the
    left edge, which reaches 512 but not 1 024; `flat` crosses every boundary along a row only)"""
    nodes, edges = line(random.Random(seed))
    s = "".join(nodes)
    return [Case(f"lead-del{d}-w{w}", "lead", (nodes, edges, s[:at] + s[at + d:]), banded(w)) for d, w, at in LEAD]


_fixed = None


def fixed_set():
    """the problems the GPU tests run, in a fixed order (built once)"""
    global _fixed
    if _fixed is None:
        _fixed = slide_cases() + flat_cases() + jump_cases() + ncol_cases() + bubble_cases() + lead_cases()
    return _fixed


def widener(seed=16):
    """A 10-base node against 2 000 random bases: whatever the band, the library's estimate of its widest row --
    min(qlen + 1, 2 w + 431 + 0.3 |longest path - qlen|) (poa_call::est_width) -- exceeds 1 000 columns, the width up to which a
    launch is k_poa_dp_t6's whatever VGA_POA_KERNEL=t7 asks for; it has few rows, so the launch order (by `footprint`) keeps it
    behind every banded problem of the fixed set."""
    rng = random.Random(seed)
    return [_seq(rng, 10)], [], _seq(rng, 2000)


def est_width(problem, params):
    """poa_call::est_width (csrc/vga_poa_run.hip); in these graphs every source-to-sink path has the same length"""
    nodes, edges, q = problem
    upto = [len(s) for s in nodes]
    for s, d in sorted(edges, key=lambda e: e[1]):
        upto[d] = max(upto[d], upto[s] + len(nodes[d]))
    longest = max(upto)
    wb, wf = params.get("wb", 10), params.get("wf", 0.01)
    w = len(q) if wb < 0 else wb + int(wf * len(q))
    return min(len(q) + 1.0, 2.0 * w + 431.0 + 0.3 * abs(longest - len(q)))


def footprint(problem, params):
    """the pool footprint estimate a call's problems are ordered by, largest first (poa_call::ensure, csrc/vga_poa_run.hip)"""
    n = sum(len(s) for s in problem[0])
    return n * est_width(problem, params) * 1.15 + ring_rows(problem) * 6.0 * (len(problem[2]) + 8.0) + 2.0 * (1 << 20)


def groups(cases):
    """[(params, [case])]: the cases by their params, in order of first appearance"""
    out = {}
    for c in cases:
        out.setdefault(tuple(sorted(c.params.items())), []).append(c)
    return [(dict(k), v) for k, v in out.items()]


# ---------------------------------------------------------------- what a kernel does with a row, from the bands alone
Row = namedtuple("Row", "r beg end simple np last")


def lds_cols(max_q):
    return ((max_q + 1 + 15) & ~15) + 16  # poa_lds_cols (vga_poa_shape.hpp:27)


def state_size(max_q):
    """poa_state_size (csrc/vga_poa_pool.hip): the state region of a launch, sized by the call's longest query"""
    maxrow = (6 * ((max_q + 8) & ~3) + 15) & ~15
    return (maxrow * (RING_SPAN + 1) + 12 * lds_cols(max_q) + 4096 + 65535) & ~65535


def ring_rows(problem):
    """poa_prob::ring_rows (poa_prepare: life + 1): the largest edge span, in nodes, that stays within the ring, plus one"""
    reach = {}
    for s, d in problem[1]:
        reach[s] = max(reach.get(s, 0), d - s)
    return max([1] + [x for x in reach.values() if x <= RING_SPAN]) + 1


def rows_of(problem, bands):
    """the rows 0..N of a problem with the band (beg, end) of each: which are simple (the only predecessor is the row above:
    poa_row_topo_of, vga_poa_row.hpp:231), how many predecessors they have, which end a node"""
    nodes, edges, _ = problem
    first, n = [], 0
    for s in nodes:
        first.append(n + 1)
        n += len(s)
    assert len(bands) == n + 1
    preds = [[] for _ in nodes]
    for s, d in edges:
        preds[d].append(first[s] + len(nodes[s]) - 1)
    out = [Row(0, bands[0][0], bands[0][1], False, 0, True)]
    for v, s in enumerate(nodes):
        for t in range(len(s)):
            r = first[v] + t
            p = [r - 1] if t else (preds[v] or [0])
            out.append(Row(r, bands[r][0], bands[r][1], p == [r - 1], len(p), t + 1 == len(s)))
    return out


def span8(row):
    """end - nbase of k_poa_dp_t6 / _t7: the last column of the row relative to the first column of its first lane"""
    return row.end - (row.beg - row.beg % T6_CPL)


def storage(row):
    """(bal, W) of poa_row_band (vga_poa_row.hpp:267): first column and width of the row's storage"""
    bal = row.beg & ~3
    return bal, (row.end - bal + 4) & ~3


def plain(query):
    return all(c in "ACGT" for c in query)


def t6_hands_back(problem, rows, max_q):
    """why k_poa_dp_t6 gives the problem up with POA_ST_RETRY (vga_poa_t6.hpp:95, :144), or None: "query" a base other than
    A / C / G / T, "ring" its fixed ring slots outgrow the state region, "window" a row that does not fit two windows"""
    if not plain(problem[2]):
        return "query"
    if T6_RING_SLOT * ring_rows(problem) > state_size(max_q):
        return "ring"
    return "window" if any(span8(x) >= 2 * T6_WIN for x in rows) else None


def t7_hands_back(problem, rows, window, max_q):
    """likewise for k_poa_dp_t7 with an LDS window of `window` columns (vga_poa_t7.hpp:88-90, :155)"""
    slot = (6 * (min(window, len(problem[2]) + 8) + 8) + 15) & ~15
    if slot * ring_rows(problem) > state_size(max_q):
        return "ring"
    return "window" if any(span8(x) + T7_PAD > window for x in rows) else None


def t6_branches(rows):
    """The register-move branch of every row k_poa_dp_t6 runs (vga_poa_t6.hpp:159-259), as (row, branch).  A simple row moves the
    row above by dl = (nbase - wbase) / 8 lanes: "dl0", "dl1-one" (DPP wave_shl, one register set), "dl1-two" (the second set
    live: the row above or this row runs a second step), "dl2+-one" / "dl2+-two" (ds_bpermute), "dl<0-one" / "dl<0-two" (the same
    else branch as dl >= 2); any other row is "staged-one" / "staged-two" (the window is rebuilt from value rows).  "alive"
    marks the first row of a second step.  The walk ends at the row that hands the problem back."""
    out, wbase, two_prev, seen_two = [], 0, False, False
    for x in rows:
        nbase = x.beg - x.beg % T6_CPL
        if x.end - nbase >= 2 * T6_WIN:
            break
        two = x.end - nbase >= T6_WIN
        if two and not seen_two:
            out.append((x.r, "alive"))
            seen_two = True
        sets = "two" if (two or two_prev) else "one"
        if x.simple:
            dl = (nbase - wbase) // T6_CPL
            out.append((x.r, "dl0" if dl == 0 else ("dl1-" if dl == 1 else "dl2+-" if dl > 1 else "dl<0-") + sets))
        elif x.r > 0:
            out.append((x.r, "staged-" + ("two" if two else "one")))
        wbase, two_prev = nbase, two
    return out


def crossing(values, at):
    """how the per-row figures of one problem stand to a threshold (a row crosses it with a figure >= at): "never", "some" or
    "all", and whether a row sits exactly on either side of it"""
    over = sum(v >= at for v in values)
    return "never" if over == 0 else "all" if over == len(values) else "some", (at - 1 in values and at in values)


def steps(width, per_step):
    return -(-width // per_step)


def wide_flips(rows, window):
    """(narrow row followed by a wide one, wide row followed by a narrow one) among the simple rows of a problem under an LDS
    window of `window` columns: the row below a wide row reads it through the far-row path"""
    nw = wn = 0
    for a, b in zip(rows, rows[1:]):
        if b.simple:
            wa, wb = storage(a)[1] + WIDE_PAD > window, storage(b)[1] + WIDE_PAD > window
            nw += (not wa) and wb
            wn += wa and not wb
    return nw, wn


def wraps(row, window):
    """a row that fits the window and straddles its wrap point (column & win_mask)"""
    bal, w = storage(row)
    return w + WIDE_PAD <= window and bal // window != (bal + w - 1) // window


def cigar_runs(cigar):
    out, num = [], ""
    for c in cigar:
        if c.isdigit():
            num += c
        else:
            out.append((int(num), c))
            num = ""
    return out


def matched_cells(res):
    """(row, column) of every match / mismatch cell of an oracle result: the cell reads H of its predecessor row one column to
    the left, which is where a lane, a step and a register set hand a word to their right neighbour"""
    out, col, pi = [], 0, 0
    for n, op in cigar_runs(res.cigar):
        for _ in range(n):
            if op == "I":
                col += 1
            else:
                if op == "M":
                    col += 1
                    out.append((res.abpoa_nodes[pi], col))
                pi += 1
    return out
