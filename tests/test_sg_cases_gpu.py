"""k_sg_mark / k_sg_emit (csrc/vga_subgraph.hip) held, bit for bit, to the plain reference of tests/sg_cases.py on the reads that
sit on their word, pass, group and budget edges: every field of every problem's tables as the kernels wrote them (VGA_SG_DUMP)
under both remain rules, the records of tests/test_gpu_parity.py's _check_align on the device route and on the host walk, and
the whole set in one batch behind a single wave on one scratch slab.  tests/test_sg_cases_cpu.py shows from the oracle alone
that the set reaches the branches it is there for."""
import pytest

import sg_cases as S
from helpers import pkg, upload_oracle_index
from test_gpu_parity import _check_align

pytestmark = pytest.mark.gpu

RULES = [(S.LONGEST_PATH, "longest-path"), (S.FIRST_EDGE, "first-out-edge")]


class _OracleOnce:
    """the oracle with map_reads and chain_anchors remembered: a batch is mapped and aligned on the CPU once per remain rule,
    however many routes and switches are held to it"""

    def __init__(self, oracle):
        self.o, self.seen = oracle, {}

    def __getattr__(self, name):
        return getattr(self.o, name)

    def chain_anchors(self, ix, query, *a, **kw):
        key = ("chain", query, a, tuple(sorted(kw.items())))
        if key not in self.seen:
            self.seen[key] = self.o.chain_anchors(ix, query, *a, **kw)
        return self.seen[key]

    def map_reads(self, ix, names, seqs, params=None):
        key = ("map", tuple(names), params.poa.remain_rule if params is not None else None)
        if key not in self.seen:
            self.seen[key] = self.o.map_reads(ix, names, seqs, params)
        return self.seen[key]


@pytest.fixture(scope="module")
def world(oracle):
    """the graph, its index on a context of this module's own, and the reference of every case under both rules"""
    spec, _, cases = S.all_cases()
    ix = oracle.Index(S.make_graph(oracle, spec), S.K)
    view = S.IndexView(ix)
    facts = [S.facts_of(oracle, ix, view, spec, c)[0] for c in cases]
    ctx = pkg().Context(0)
    upload_oracle_index(ctx, ix)
    yield dict(cases=cases, ix=ix, facts=facts, ctx=ctx, once=_OracleOnce(oracle), alone={})
    ctx.close()


def records(path):
    return S.parse_dump(path.read_text())


def payload(rec):
    return {k: v for k, v in rec.items() if k not in ("problem", "read")}


def align_dumped(world, idx, rule, monkeypatch, dump, check=True):
    """the reads `idx` of the set as one batch on the device route, with the tables dumped: (align result, [record])"""
    reads = [world["cases"][i].read for i in idx]
    monkeypatch.setenv("VGA_SG_DUMP", str(dump))
    if check:
        al = _check_align(world["once"], world["ctx"], world["ix"], reads, remain_rule=rule)
    else:
        pp = pkg().default_poa_params()
        pp.remain_rule = rule
        b = world["ctx"].batch([r.seq for r in reads])
        al = b.align(b.map(), params=pp)
    monkeypatch.delenv("VGA_SG_DUMP")
    recs = records(dump)
    assert sorted(r["read"] for r in recs) == list(range(len(idx))), "one record per read"
    assert [r["problem"] for r in recs] == list(range(len(idx))), "records in launch order"
    return al, recs


def hold_to_reference(world, idx, rule, recs):
    """every field of every record against the reference of the read it names, and its sg_desc against the chain's"""
    bad = []
    for rec in recs:
        f = world["facts"][idx[rec["read"]]]
        if rec["desc"] != tuple(f.desc[k] for k in S.DESC_FIELDS):
            bad.append((f.case.name, "desc", rec["desc"], f.desc))
        bad += [(f.case.name,) + d for d in S.differences(rec, f.ref[rule])]
    assert not bad, (len(bad), bad[:8])


@pytest.mark.parametrize("rule", [r for r, _ in RULES], ids=[n for _, n in RULES])
@pytest.mark.parametrize("fam", S.FAMILIES)
def test_tables_of_the_family_equal_the_reference(world, monkeypatch, tmp_path, fam, rule):
    """One batch per family.  The dump of every problem -- handles, first rows, predecessor list, sinks, the four words of every
    table entry and of the source entry, the sequence bytes, n_nodes, N, n_preds, n_sinks, wlo, whi, longest, life, flags --
    equals the reference, matched by the record's read number; the alignment records, poa_rows and poa_cells equal the
    oracle's on the device route and on the host walk, and the two routes agree."""
    idx = [i for i, c in enumerate(world["cases"]) if c.family == fam]
    al, recs = align_dumped(world, idx, rule, monkeypatch, tmp_path / "sg.txt")
    hold_to_reference(world, idx, rule, recs)
    if fam == "n4":
        # every residue of N % 4 in front of another problem of the part: the next seq0 is rounded up from it
        assert {r["N"] % 4 for r in recs[:-1]} == {0, 1, 2, 3}
    monkeypatch.setenv("VGA_SUBGRAPH", "host")
    host = _check_align(world["once"], world["ctx"], world["ix"], [world["cases"][i].read for i in idx], remain_rule=rule)
    assert (host.cigar, host.cs, host.path_handles.tolist(), host.poa_rows, host.poa_cells) == (
        al.cigar, al.cs, al.path_handles.tolist(), al.poa_rows, al.poa_cells)


def alone(world, i, monkeypatch, tmp_path):
    """the dump of case i as the only problem of a call (default remain rule), taken once"""
    if i not in world["alone"]:
        _, recs = align_dumped(world, [i], S.FIRST_EDGE, monkeypatch, tmp_path / ("alone%d.txt" % i), check=False)
        world["alone"][i] = recs[0]
    return world["alone"][i]


@pytest.mark.parametrize("split", ["1", "0"])
def test_all_families_in_one_batch_behind_one_wave(world, monkeypatch, tmp_path, split):
    """VGA_SG_SPLIT=1 VGA_SG_SIDE_WAVES=1: the first problem of the launch order is the store's first part; one wave serves all the
    others, one after another, on one scratch slab -- `best` and `stamp` of a walk, then the wb_* / rf overlay of k_sg_emit, then
    the next chain's walk.  VGA_SG_SPLIT=0: one part, a wave per problem.  Either way every problem's tables equal the reference
    and the dump it had as the only problem of a call, and the records equal the oracle's."""
    cases = world["cases"]
    idx = list(range(len(cases)))
    assert len(idx) >= 40 and {c.family for c in cases} == set(S.FAMILIES)
    monkeypatch.setenv("VGA_SG_SPLIT", split)
    monkeypatch.setenv("VGA_SG_SIDE_WAVES", "1")
    _, recs = align_dumped(world, idx, S.FIRST_EDGE, monkeypatch, tmp_path / "mixed.txt")
    monkeypatch.delenv("VGA_SG_SPLIT")
    monkeypatch.delenv("VGA_SG_SIDE_WAVES")
    hold_to_reference(world, idx, S.FIRST_EDGE, recs)
    differ = [cases[r["read"]].name for r in recs if payload(r) != payload(alone(world, r["read"], monkeypatch, tmp_path))]
    assert not differ, differ
