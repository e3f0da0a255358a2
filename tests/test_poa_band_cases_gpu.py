"""The POA kernels on the column axis of the DP -- the problems of tests/poa_band_cases.py, whose bands sit exactly at and either
side of the lane, step and window thresholds of k_poa_dp_t4 / _t5 / _t6 / _t7 / _lds -- held to the oracle bit for bit with the
assertions of tests/test_gpu_parity.py under every switch that reaches another DP or traceback kernel.  On top of parity, from
the launch trace (VGA_TRACE): the launch has the kernel, workgroup size and window the configuration pinned, and the specialised
kernels hand back exactly the problems that the predicates of poa_band_cases say leave their window; and, row by row, the bands
of VGA_POA_DUMP_ROWS equal the oracle's OG_POA_ROWS.  tests/test_poa_band_cases_cpu.py shows from the oracle alone that the set
reaches the branches it is there for."""
import re

import pytest

import poa_band_cases as B
from helpers import pkg
from test_gpu_parity import _check_poa
from test_poa_topology_gpu import _OracleOnce, both_params

pytestmark = pytest.mark.gpu

WIDENER = B.widener()


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


class _OracleRows(_OracleOnce):
    """_OracleOnce that also keeps the band of every row (OG_POA_ROWS) of the one alignment it runs per problem"""

    def __init__(self, oracle):
        super().__init__(oracle)
        self.bands = {}

    @staticmethod
    def key(nodes, edges, q, params):
        return (id(nodes), id(edges), q) + (tuple(getattr(params, f[0]) for f in params._fields_) if params is not None else ())

    def poa_align(self, nodes, edges, q, params=None):
        k = self.key(nodes, edges, q, params)
        if k not in self.seen:
            res, self.bands[k] = self.o.poa_align_rows(nodes, edges, q, params)
            self.seen[k] = (nodes, edges, res)
        return self.seen[k][2]

    def rows(self, problem, params):
        self.poa_align(*problem, params)
        return B.rows_of(problem, self.bands[self.key(*problem, params)])


@pytest.fixture(scope="module")
def once(oracle):
    return _OracleRows(oracle)


# ---------------------------------------------------------------- the launch trace
LAUNCH = re.compile(r"launch (\d+) problems, NT (\d+), (k_poa_dp_\w+), window (\d+) of (\d+) columns")
T7 = re.compile(r"k_poa_dp_t7<(\d+)>: window (\d+) columns")
HANDED = re.compile(r"poa: (\d+) problems handed back by the specialised DP kernel")


def launches_of(trace):
    """([launch], problems handed back): a launch is {n, nt, family, window, cols, special}; special is None for the family's own
    kernel, ("t6",) or ("t7", NT, window)"""
    out, handed = [], 0
    for ln in trace.splitlines():
        m = LAUNCH.search(ln)
        if m:
            out.append(dict(n=int(m.group(1)), nt=int(m.group(2)), family=m.group(3), window=int(m.group(4)), cols=int(m.group(5)), special=None))
        elif "k_poa_dp_t6<8>" in ln:
            out[-1]["special"] = ("t6",)
        elif T7.search(ln):
            out[-1]["special"] = ("t7",) + tuple(int(x) for x in T7.search(ln).groups())
        m = HANDED.search(ln)
        if m:
            handed += int(m.group(1))
    return out, handed


def expected_hand_backs(once, problems, oparams, special):
    """the problems of one call that the kernel `special` gives up, by the CPU predicates (the state region is sized by the call's
    longest query)"""
    if special is None:
        return []
    max_q = max(len(p[2]) for p in problems)
    why = [B.t6_hands_back(p, once.rows(p, oparams), max_q) if special[0] == "t6" else B.t7_hands_back(p, once.rows(p, oparams), special[2], max_q)
           for p in problems]
    return [w for w in why if w]


def run_config(once, ctx, capfd, monkeypatch, env, cases, pin, **kw):
    """Every group of `cases` (the problems of equal band parameters are one call) under `env`: parity, the pinned shape, and
    the hand-backs.  pin: dict(family=, nt=, window=, special=) -- what every first launch of a call must show; window is the
    pinned VGA_POA_WINDOW, which only applies to a call whose column codes outgrow it.  Returns the hand-backs seen, by reason."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VGA_TRACE", "1")
    seen = {}
    for band, group in B.groups(cases):
        problems = [c.problem for c in group]
        if (pin.get("special") or (None,))[0] == "t7" and max(B.est_width(p, band) for p in problems) <= 1000:
            problems = problems + [WIDENER]  # (k_poa_dp_t6 would take the launch: poa_band_cases.widener)
        pp, op = both_params(once, **dict(band, **kw))
        capfd.readouterr()
        _check_poa(once, ctx, problems, pp, op)
        launches, handed = launches_of(capfd.readouterr().err)
        tag = (band, launches)
        assert launches and launches[0]["n"] == len(problems), tag
        first, rest = launches[0], launches[1:]
        if "family" in pin:
            assert first["family"] == pin["family"], tag
        if "nt" in pin:
            assert first["nt"] == pin["nt"], tag
        if "window" in pin:
            assert first["window"] == (pin["window"] if pin["window"] < first["cols"] else first["cols"]), tag
        if "special" in pin:
            assert first["special"] == pin["special"], tag
        # hand-backs, exactly: the trace's count, and the re-run -- one launch of the general kernel with just those problems
        want = expected_hand_backs(once, problems, op, first["special"])
        assert handed == len(want), (tag, want)
        assert [(x["n"], x["special"]) for x in rest] == ([(len(want), None)] if want else []), (tag, want)
        for w in want:
            seen[w] = seen.get(w, 0) + 1
    return seen


def ident(env):
    return ",".join("%s=%s" % kv for kv in env.items()) or "default"


T5, T4, LDS = "k_poa_dp_t5", "k_poa_dp_t4", "k_poa_dp_lds"
CONFIGS = [({}, {"family": T5})]
CONFIGS += [({"VGA_POA_KERNEL": "t5", "VGA_POA_NT": str(nt)}, {"family": T5, "nt": nt, "special": None}) for nt in (128, 256, 512)]
CONFIGS += [({"VGA_POA_KERNEL": "t5", "VGA_POA_NT": "128", "VGA_POA_WINDOW": str(w)}, {"family": T5, "nt": 128, "window": w, "special": None})
            for w in (256, 512, 1024)]
CONFIGS += [({"VGA_POA_KERNEL": "t4", "VGA_POA_NT": str(nt)}, {"family": T4, "nt": nt, "special": None}) for nt in (128, 256)]
CONFIGS += [({"VGA_POA_KERNEL": "t4", "VGA_POA_NT": str(nt), "VGA_POA_WINDOW": "256"}, {"family": T4, "nt": nt, "window": 256, "special": None})
            for nt in (128, 256)]
CONFIGS += [({"VGA_POA_KERNEL": k}, {"family": T5, "special": ("t6",)}) for k in ("t6", "t6,generic")]
CONFIGS += [({"VGA_POA_KERNEL": "t7", "VGA_POA_T7_NT": str(nt), "VGA_POA_T7_WINDOW": str(w)}, {"family": T5, "special": ("t7", nt, w)})
            for nt, w in ((128, 1024), (128, 4096), (256, 4096))]
CONFIGS += [({"VGA_POA_KERNEL": "unpacked,%d" % nt}, {"family": LDS, "nt": nt, "special": None}) for nt in (128, 256)]
CONFIGS += [({"VGA_POA_TB": "wave"}, {"family": T5, "special": None}), ({"VGA_POA_ARENAS": "0"}, {"family": T5, "special": None})]


@pytest.mark.parametrize("env,pin", CONFIGS, ids=[ident(e) for e, _ in CONFIGS])
def test_fixed_set_under_the_kernel_switches(once, ctx, capfd, monkeypatch, env, pin):
    """Steps of 4 NT columns (k_poa_dp_t5 and _t4 with 128, 256 and 512 threads, k_poa_dp_lds as `unpacked` with 128 and 256), LDS
    windows of 256, 512 and 1 024 columns (wide rows on the HBM detour next to narrow ones, the wrap point), k_poa_dp_t6 with
    and without the default-penalty specialisation, k_poa_dp_t7 with a window that some problems leave and with one that
    holds them all, at 128 and 256 threads (one and two steps of 8 NT columns), the traceback kernel of its own and the classic
    pool.  The hand-backs of the specialised kernels are exact: k_poa_dp_t6 gives up the 26 queries that hold an N and the
    problems with a row beyond two windows, k_poa_dp_t7 those with a row beyond its window, nobody anything else."""
    seen = run_config(once, ctx, capfd, monkeypatch, env, B.fixed_set(), pin)
    special = pin.get("special")
    if special == ("t6",):
        assert seen.get("query") == 26 and seen.get("window", 0) >= 10 and set(seen) == {"query", "window"}, seen
    elif special and special[2] == 1024:
        assert seen.get("window", 0) >= 20 and set(seen) == {"window"}, seen
    elif "special" in pin:
        assert not seen, seen


def reduced():
    keep = re.compile(r"slide-w(124|251|253|507|509)$|jump-(ins8|ins33|ins600|del24|del65|del200)-(w200|w253)$")
    return [c for c in B.fixed_set() if keep.match(c.name)]


@pytest.mark.parametrize("kw,family", [(dict(gap_open1=31, gap_ext1=33), T4), (dict(gap_open2=200), LDS)], ids=[T4, LDS])
def test_sliding_and_jumping_bands_under_other_penalty_families(once, ctx, capfd, monkeypatch, kw, family):
    """a first gap piece of open + extend = 64 is k_poa_dp_t4's and a second one that needs 2-byte deltas k_poa_dp_lds's (its own
    step loop): reached by the choice of family, not by a switch, on a reduced set of sliding and jumping bands"""
    cases = reduced()
    assert len(cases) == 5 + 12
    assert not run_config(once, ctx, capfd, monkeypatch, {}, cases, {"family": family, "special": None}, **kw)


def test_fixed_set_under_the_longest_path_remain_rule(once, ctx, capfd, monkeypatch):
    """every source-to-sink path of these graphs has the same length, so the band is the same under either rule: the hand-backs
    of the default selection (k_poa_dp_t6 on the launches of narrow estimates) are counted all the same"""
    run_config(once, ctx, capfd, monkeypatch, {}, B.fixed_set(), {"family": T5}, remain_rule=0)


# ---------------------------------------------------------------- per-row bands
DUMPED = ("slide-w123", "slide-w251", "slide-w253", "slide-w505", "slide-w507", "slide-w509", "flat-q252", "flat-q512", "flat-q1016", "flat-q1024",
          "jump-ins33-w253", "jump-ins600-default", "jump-del65-w200", "ncol-w253-all", "bubble-w253", "bubble-w509", "lead-del560-w462")
DUMP_CONFIGS = [({"VGA_POA_KERNEL": "t5", "VGA_POA_NT": "128", "VGA_POA_WINDOW": "512"}, None, False), ({"VGA_POA_KERNEL": "t6"}, ("t6",), False),
                ({"VGA_POA_KERNEL": "t7", "VGA_POA_T7_NT": "128", "VGA_POA_T7_WINDOW": "4096"}, ("t7", 128, 4096), False),
                ({"VGA_POA_KERNEL": "t7", "VGA_POA_T7_NT": "128", "VGA_POA_T7_WINDOW": "1024"}, ("t7", 128, 1024), True)]


@pytest.mark.parametrize("env,special,alone", DUMP_CONFIGS, ids=[ident(e) for e, _, _ in DUMP_CONFIGS])
def test_band_of_every_row_equals_the_oracle(once, ctx, capfd, monkeypatch, tmp_path, env, special, alone):
    """One problem of each family and at each threshold, first in its call: beg and end of every row as the kernel stored them
    (VGA_POA_DUMP_ROWS: the first problem of the launch that ran last) against OG_POA_ROWS.  The sum of band cells that
    _check_poa compares cannot tell two compensating rows apart; this can.  lmax and rmax are only stored on some rows and are
    not compared.  For a problem that the specialised kernel handed back the dump is that of the re-run in k_poa_dp_t5: so it
    is for five problems under k_poa_dp_t6 and for all of them under k_poa_dp_t7 with 1 024 columns.  Under k_poa_dp_t7 a
    problem of a narrow estimate needs the widener next to it, behind it in the launch order: the two unbanded problems whose
    footprint is below the widener's are left to the other configurations; and with a window of 1 024 columns the widener is
    handed back and would head the re-run, so that configuration takes the problems that reach k_poa_dp_t7 alone."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VGA_TRACE", "1")
    dump = tmp_path / "rows.txt"
    monkeypatch.setenv("VGA_POA_DUMP_ROWS", str(dump))
    by_name = {c.name: c for c in B.fixed_set()}
    ran = []
    for name in DUMPED:
        c = by_name[name]
        problems = [c.problem]
        if special and special[0] == "t7" and B.est_width(c.problem, c.params) <= 1000:
            if alone or B.footprint(c.problem, c.params) <= B.footprint(WIDENER, c.params):
                continue
            problems.append(WIDENER)
        pp, op = both_params(once, **c.params)
        capfd.readouterr()
        _check_poa(once, ctx, problems, pp, op)
        launches, handed = launches_of(capfd.readouterr().err)
        assert launches[0]["special"] == special, (name, launches)
        rows = once.rows(c.problem, op)
        got = [tuple(int(x) for x in ln.split()[:3]) for ln in dump.read_text().splitlines()]
        want = [(x.r, x.beg, x.end) for x in rows]
        diff = [(g, w) for g, w in zip(got, want) if g != w]
        assert len(got) == len(want) and not diff, (name, len(got), len(want), diff[:5])
        ran.append(name)
    left_out = set(DUMPED) - set(ran)
    if alone:
        assert set(ran) == {"slide-w505", "slide-w507", "slide-w509", "flat-q1016", "flat-q1024", "bubble-w509", "lead-del560-w462"}
    else:
        assert left_out == ({"flat-q252", "flat-q512"} if special and special[0] == "t7" else set())
