"""The POA problems of tests/poa_band_cases.py on the CPU: (1) the fixed set the GPU tests run reaches, judged from the oracle's
per-row bands (OG_POA_ROWS) and CIGARs alone, every branch of the DP kernels' column axis it is there for -- a condition on the
fixtures: no cell may be empty, and the table of cell -> case names is printed (pytest -s); (2) the oracle is the true optimum on
small members, against the path-enumerating general-gap programme of test_oracle_poa_cpu.py."""
import random
import re

import pytest

import poa_band_cases as B
from test_oracle_poa_cpu import all_paths, wsb_global

WINDOWS = (256, 512, 1024)


def params_of(oracle, kw):
    p = oracle.default_poa_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def refs(oracle):
    """(oracle result, rows with their bands) of every problem of the fixed set"""
    out = []
    for c in B.fixed_set():
        res, bands = oracle.poa_align_rows(*c.problem, params_of(oracle, c.params))
        out.append((res, B.rows_of(c.problem, bands)))
    return out


def show(title, cells):
    print(f"\n{title}")
    for k in sorted(cells, key=str):
        names = sorted(set(cells[k]))
        print(f"  {k}: {len(names)} -- {', '.join(names[:6])}{' ...' if len(names) > 6 else ''}")


def test_generators_are_seeded_and_well_formed():
    a = B.fixed_set()
    b = B.slide_cases() + B.flat_cases() + B.jump_cases() + B.ncol_cases() + B.bubble_cases() + B.lead_cases()
    assert [(c.name, c.problem, c.params) for c in a] == [(c.name, c.problem, c.params) for c in b]
    assert len({c.name for c in a}) == len(a) and 120 <= len(a) <= 160
    for c in a:
        nodes, edges, q = c.problem
        assert q and all(nodes) and all(0 <= s < d < len(nodes) for s, d in edges) and len(set(edges)) == len(edges), c.name
        assert sum(len(s) for s in nodes) <= 1600 and len(q) <= 2200 and set(c.params) <= {"wb", "wf"}, c.name
    fam = {f: [c for c in a if c.family == f] for f in ("slide", "flat", "jump", "ncol", "bubble", "lead")}
    assert sum(len(v) for v in fam.values()) == len(a)
    assert [c.params["wb"] for c in fam["slide"]] == list(B.SLIDE_W) and all(c.params["wf"] == 0 for c in fam["slide"])
    assert all("".join(c.problem[0]) == c.problem[2] and all(len(s) == B.LINE_NODE for s in c.problem[0]) for c in fam["slide"])
    assert [len(c.problem[2]) for c in fam["flat"]] == list(B.FLAT_QLEN) and all(c.params == {"wb": -1} for c in fam["flat"])
    assert all("".join(c.problem[0]) in c.problem[2] and len(c.problem[0]) == 2 for c in fam["flat"])
    assert len(fam["jump"]) == 3 * (len(B.JUMP_INS) + len(B.JUMP_DEL)) and len(fam["ncol"]) == 2 * (len(B.NCOL_COLS) + 1)
    for c in fam["ncol"]:
        at = [i + 1 for i, ch in enumerate(c.problem[2]) if ch == "N"]  # columns
        want = sorted({len(c.problem[2]) if x < 0 else max(x, 1) for x in B.NCOL_COLS})
        assert at == want if c.name.endswith("-all") else (len(at) == 1 and at[0] in want), c.name
    assert plain_everywhere_else(a)
    assert len(B.groups(a)) == len({tuple(sorted(c.params.items())) for c in a})


def plain_everywhere_else(cases):
    return all(B.plain(c.problem[2]) for c in cases if c.family != "ncol") and all(B.plain("".join(c.problem[0])) for c in cases)


def test_predicates_on_hand_made_rows():
    """a line of 2 + 1 bases and a SNP bubble; bands chosen by hand"""
    prob = (["AC", "G", "T", "A"], [(0, 1), (0, 2), (1, 3), (2, 3)], "ACGA")
    rows = B.rows_of(prob, [(0, 4), (0, 4), (8, 519), (16, 528), (40, 600), (32, 1055)])
    assert [(x.simple, x.np, x.last) for x in rows] == [(False, 0, True), (True, 1, False), (True, 1, True), (True, 1, True), (False, 1, True),
                                                         (False, 2, True)]
    assert [B.span8(x) for x in rows] == [4, 4, 511, 512, 560, 1023] and B.storage(rows[4]) == (40, 564) and B.storage(rows[1]) == (0, 8)
    assert B.t6_branches(rows) == [(1, "dl0"), (2, "dl1-one"), (3, "alive"), (3, "dl1-two"), (4, "staged-two"), (5, "staged-two")]
    assert B.t6_hands_back(prob, rows, 4) is None and B.t7_hands_back(prob, rows, 1024, 4) == "window" and B.t7_hands_back(prob, rows, 4096, 4) is None
    assert B.t6_hands_back((prob[0], prob[1], "ACNA"), rows, 4) == "query"
    rows[5] = rows[5]._replace(end=1056)
    assert B.t6_hands_back(prob, rows, 4) == "window" and B.t6_branches(rows)[-1] == (4, "staged-two")
    assert B.ring_rows(prob) == 3 and B.ring_rows((["A"], [], "A")) == 2 and (B.state_size(200), B.state_size(300)) == (65536, 131072)
    assert B.crossing([510, 511, 512], 512) == ("some", True) and B.crossing([3, 4], 512) == ("never", False) and B.crossing([600], 512) == ("all", False)
    assert B.wide_flips(rows[:4], 256) == (1, 0) and B.wraps(B.Row(9, 250, 300, True, 1, False), 256) and not B.wraps(B.Row(9, 256, 300, True, 1, False), 256)
    assert B.cigar_runs("3M20I1M") == [(3, "M"), (20, "I"), (1, "M")] and (B.steps(512, 512), B.steps(516, 512)) == (1, 2)


def test_every_problem_aligns(refs):
    for c, (res, rows) in zip(B.fixed_set(), refs):
        assert res.ok and len(rows) == res.n_rows + 1, c.name


def test_k_poa_dp_t6_register_moves_second_step_and_hand_back(refs):
    """Every way k_poa_dp_t6 moves the row above when the window base moves, with one and with two register sets; a problem whose
    second set comes alive after row 0; at the 512-column (second step) and 1 024-column (hand-back) thresholds a problem that
    never crosses, one in which only some rows cross, and one with rows exactly at the threshold (end - nbase = 511 | 512 and
    1 023 | 1 024).  dl < 0 (the band's left edge moves left past a lane) takes the same `else` branch as dl >= 2 and is not
    required: whether the set has it is printed.  Staged rows (behind a SNP bubble) fall on every phase beg % 8."""
    cells, phases = {}, set()
    for c, (res, rows) in zip(B.fixed_set(), refs):
        by_row = dict((x.r, x) for x in rows)
        br = B.t6_branches(rows)
        for r, b in br:
            if b == "alive":
                b = "alive at row 0" if r == 0 else "alive after row 0"
            cells.setdefault(b, []).append(c.name)
            if b.startswith("staged"):
                phases.add(by_row[r].beg % 8)
        x = [B.span8(r) for r in rows]
        for at in (B.T6_WIN, 2 * B.T6_WIN):
            how, exact = B.crossing(x, at)
            cells.setdefault((at, how), []).append(c.name)
            if exact:
                cells.setdefault((at, "exact"), []).append(c.name)
    show("k_poa_dp_t6: branch -> problems", cells)
    print("  dl < 0 occurs:", sorted(k for k in cells if str(k).startswith("dl<0")))
    for b in ("dl0", "dl1-one", "dl1-two", "dl2+-one", "dl2+-two", "staged-one", "staged-two", "alive after row 0"):
        assert cells.get(b), b
    for at in (512, 1024):
        for how in ("never", "some", "exact"):
            assert cells.get((at, how)), (at, how)
    assert phases == set(range(8)), phases


def test_k_poa_dp_t6_and_t7_hand_back_reasons(refs):
    """what the GPU tests count: problems that leave k_poa_dp_t6 for a query base other than A / C / G / T and for a row beyond two
    windows, problems that leave k_poa_dp_t7's window of 1 024 columns (and none that leaves 4 096), and no problem whose ring
    outgrows the state region (poa_state_size: the queries are long enough for 64 KiB and the edges span at most two nodes)"""
    cells = {}
    for c, (res, rows) in zip(B.fixed_set(), refs):
        q = len(c.problem[2])
        cells.setdefault(("t6", B.t6_hands_back(c.problem, rows, q)), []).append(c.name)
        for w in (1024, 4096):
            cells.setdefault(("t7", w, B.t7_hands_back(c.problem, rows, w, q)), []).append(c.name)
    show("hand-backs: (kernel, [window,] reason) -> problems", cells)
    assert cells.get(("t6", "query")) and cells.get(("t6", "window")) and cells.get(("t6", None)) and not cells.get(("t6", "ring"))
    assert cells.get(("t7", 1024, "window")) and cells.get(("t7", 1024, None))
    assert set(k[2] for k in cells if k[:2] == ("t7", 4096)) == {None}
    assert len(cells[("t7", 1024, "window")]) > len(cells[("t6", "window")])  # (1 016 .. 1 023: t7's window only)


def test_k_poa_dp_t7_window_and_steps(refs):
    """the three-way split at k_poa_dp_t7's window of 1 024 columns (it hands back when end - nbase + 9 > window: 1 015 | 1 016), and
    rows of one and of two steps of 8 NT columns at NT = 128 and NT = 256"""
    cells = {}
    for c, (res, rows) in zip(B.fixed_set(), refs):
        x = [B.span8(r) for r in rows]
        how, exact = B.crossing(x, 1024 - B.T7_PAD + 1)
        cells.setdefault(("window 1024", how), []).append(c.name)
        if exact:
            cells.setdefault(("window 1024", "exact"), []).append(c.name)
        for nt in (128, 256):
            for n in {v // (B.T6_CPL * nt) + 1 for v in x}:  # (vga_poa_t7.hpp: for (c0 = 0; nbase + c0 <= end; c0 += STEP))
                cells.setdefault((f"NT {nt}", f"{n} steps"), []).append(c.name)
    show("k_poa_dp_t7: cell -> problems", cells)
    for how in ("never", "some", "exact"):
        assert cells.get(("window 1024", how)), how
    for nt in (128, 256):
        assert cells.get((f"NT {nt}", "1 steps")) and cells.get((f"NT {nt}", "2 steps")), nt


def test_k_poa_dp_t4_t5_and_lds_steps_wide_rows_and_wrap(refs):
    """storage widths W of exactly 4 NT - 4, 4 NT and 4 NT + 4 columns (NT = 128, 256: the last lane of a step, one step exactly,
    the first lane of a second step -- k_poa_dp_lds<NT, 4> steps by the same 4 NT columns); under LDS windows of 256, 512 and
    1 024 columns a wide row (W + 8 > window: the HBM detour) below a narrow one and a narrow row below a wide one; a row
    that fits the window and straddles its wrap point.  A window only applies to a query whose column codes outgrow it."""
    cells = {}
    for c, (res, rows) in zip(B.fixed_set(), refs):
        widths = {B.storage(r)[1] for r in rows}
        for nt in (128, 256):
            for d in (-4, 0, 4):
                if B.T4_CPL * nt + d in widths:
                    cells.setdefault((f"NT {nt}", f"W = 4 NT {d:+d}", f"{B.steps(B.T4_CPL * nt + d, B.T4_CPL * nt)} steps"), []).append(c.name)
        for w in WINDOWS:
            if B.lds_cols(len(c.problem[2])) <= w:
                continue
            nw, wn = B.wide_flips(rows, w)
            if nw:
                cells.setdefault((f"window {w}", "narrow then wide"), []).append(c.name)
            if wn:
                cells.setdefault((f"window {w}", "wide then narrow"), []).append(c.name)
            if any(B.wraps(r, w) for r in rows):
                cells.setdefault((f"window {w}", "wraps"), []).append(c.name)
            flat = c.family == "flat" and len(widths) == 1
            if flat:
                cells.setdefault((f"window {w}", "every row wide" if min(widths) + B.WIDE_PAD > w else "every row narrow"), []).append(c.name)
    show("k_poa_dp_t4 / _t5 / _lds: cell -> problems", cells)
    for nt in (128, 256):
        assert cells.get((f"NT {nt}", "W = 4 NT -4", "1 steps")) and cells.get((f"NT {nt}", "W = 4 NT +0", "1 steps")), nt
        assert cells.get((f"NT {nt}", "W = 4 NT +4", "2 steps")), nt
    for w in WINDOWS:
        for what in ("narrow then wide", "wide then narrow", "wraps", "every row wide", "every row narrow"):
            assert cells.get((f"window {w}", what)), (w, what)


def test_optimal_path_crosses_step_and_register_set_boundaries(refs):
    """A kernel that is wrong in a cell the optimal path does not touch still gets score and CIGAR right.  So the path itself
    has to cross: a matched cell in the first column of a later step reads the word its left neighbour parked (k_poa_dp_t4 /
    _t5 / _lds: column bal + 4 NT, NT = 128 and 256), lane 0 of k_poa_dp_t6's second register set reads lane 63 of the first
    (column nbase + 512), the first lane of k_poa_dp_t7's second step the last lane of the first (nbase + 8 NT, NT = 128); and
    the cell before each of them is matched too, so the path enters it on the diagonal"""
    cells = {}
    for c, (res, rows) in zip(B.fixed_set(), refs):
        path = set(B.matched_cells(res))
        for r, j in path:
            if (r - 1, j - 1) not in path or not rows[r].simple:
                continue
            bal, nbase = B.storage(rows[r])[0], rows[r].beg - rows[r].beg % B.T6_CPL
            for nt in (128, 256):
                if j - bal == B.T4_CPL * nt:
                    cells.setdefault(f"first column of the second step of 4 x {nt}", []).append(c.name)
            if j - nbase == B.T6_WIN and B.t6_hands_back(c.problem, rows, len(c.problem[2])) is None:
                cells.setdefault("lane 0 of k_poa_dp_t6's second set", []).append(c.name)
            if j - nbase == B.T6_CPL * 128:
                cells.setdefault("first column of the second step of 8 x 128", []).append(c.name)
    show("the optimal path enters on the diagonal: cell -> problems", cells)
    assert len(cells) == 4 and all(any(n.startswith("lead") or n.startswith("slide") for n in v) for v in cells.values()), cells


def test_insertion_and_deletion_runs_survive_the_band(refs):
    """the traceback stages 32 columns and up to 64 rows at a time: an insertion run of every length of JUMP_INS and a deletion
    run of every length of JUMP_DEL is in the oracle's CIGAR, under each of the three bands; the unbanded problems hold two
    insertion runs of a hundred bases and more each"""
    cells = {}
    for c, (res, rows) in zip(B.fixed_set(), refs):
        runs = B.cigar_runs(res.cigar)
        if c.family == "jump":
            m = re.match(r"jump-(ins|del)(\d+)-(\w+)$", c.name)
            want = (int(m.group(2)), "I" if m.group(1) == "ins" else "D")
            assert want in runs and sum(1 for _, op in runs if op != "M") == 1, (c.name, res.cigar)
            cells.setdefault((m.group(3), want[1]), []).append(want[0])
        if c.family == "flat":
            assert sum(1 for n, op in runs if op == "I" and n >= 100) == 2, (c.name, res.cigar)
    print("\ntraceback: (band, operation) -> run lengths in the oracle's CIGARs")
    for k in sorted(cells):
        print(f"  {k}: {sorted(cells[k])}")
    for band, _ in B.JUMP_BANDS:
        assert sorted(cells[(band, "I")]) == sorted(B.JUMP_INS) and sorted(cells[(band, "D")]) == sorted(B.JUMP_DEL), band


def test_widener_keeps_a_launch_from_the_one_wave_kernel():
    """poa_choose_shape gives a launch to k_poa_dp_t6 whatever VGA_POA_KERNEL=t7 asks for while the width estimates stay at or below
    1 000 columns: the GPU tests add `widener()` to such a call.  Its estimate is above under every band of the set; its footprint
    estimate is below that of the banded problems, which keeps it from the head of their launches (the launch order)"""
    w = B.widener()
    for kw, cases in B.groups(B.fixed_set()):
        assert B.est_width(w, kw) > 1000
        for c in cases:
            assert c.family == "flat" or B.footprint(w, kw) < B.footprint(c.problem, kw), c.name
    narrow = [c.name for c in B.fixed_set() if B.est_width(c.problem, c.params) <= 1000]
    assert narrow and len(narrow) < len(B.fixed_set())


# ---------------------------------------------------------------- the oracle is the optimum on small members
def small_members(rng):
    out = [c.problem + ({"wb": -1},) for c in B.fixed_set() if c.family == "flat" and len(c.problem[2]) <= 252]
    nodes, edges = B.line(rng, 60, 20)
    for _, q in B.jump_queries(rng, nodes, at=30, ins=(7, 8, 9, 15, 16, 17, 31, 32, 33, 40), dels=(23, 24, 25)):
        out += [(nodes, edges, q, {"wb": -1}), (nodes, edges, q, {"wb": 200, "wf": 0.0})]
    return out


def test_oracle_score_is_the_optimum_on_small_flat_and_jump_members(oracle):
    """under the default penalties; a band of 200 columns either side holds every column of these problems"""
    m, x, o1, e1, o2, e2 = 2, 4, 4, 2, 24, 1
    g = lambda k: min(o1 + k * e1, o2 + k * e2)
    problems = small_members(random.Random(21))
    assert len(problems) == 4 + 2 * 13
    cache = {}
    for nodes, edges, q, kw in problems:
        paths = all_paths(len(nodes), edges)
        assert len(paths) == 1
        s = "".join(nodes[v] for v in paths[0])
        if (s, q) not in cache:
            cache[(s, q)] = wsb_global(s, q, m, x, g)
        r = oracle.poa_align(nodes, edges, q, params_of(oracle, kw))
        assert r.ok and r.best_score == cache[(s, q)], (nodes, q, kw, r.best_score, cache[(s, q)], r.cigar)
