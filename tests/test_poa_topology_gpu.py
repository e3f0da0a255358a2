"""The POA kernels on the graph shapes of tests/poa_topologies.py -- joins of more than four predecessors (the traceback stages
four predecessor rows per lane and reads the others from memory; DRB1-3123 has a maximum in-degree of exactly 4), value rows
read more than POA_RING_SPAN nodes ahead (kept outside the ring: the boundary 32 | 33), several sources and sinks -- held to
the oracle bit for bit with the assertions of tests/test_gpu_parity.py, under every switch that reaches another DP or
traceback kernel, through vga_poa_batch and through vga_align_batch.  tests/test_poa_topology_cpu.py shows from the oracle
alone that the fixed set reaches those branches."""
import ctypes as C

import pytest

import poa_topologies as T
from helpers import pkg, upload_oracle_index
from test_coverage_gpu import same, walker
from test_gpu_parity import _check_align, _check_poa

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


class _OracleOnce:
    """the oracle with poa_align remembered: a problem of the fixed set is aligned once per parameter set, whatever the number of
    kernel configurations that are held to it.  (The problems live as long as the module, so their ids name them.)"""

    def __init__(self, oracle):
        self.o, self.seen = oracle, {}

    def __getattr__(self, name):
        return getattr(self.o, name)

    def poa_align(self, nodes, edges, q, params=None):
        key = (id(nodes), id(edges), q) + (tuple(getattr(params, f[0]) for f in params._fields_) if params is not None else ())
        if key not in self.seen:
            self.seen[key] = (nodes, edges, self.o.poa_align(nodes, edges, q, params))
        return self.seen[key][2]


@pytest.fixture(scope="module")
def once(oracle):
    return _OracleOnce(oracle)


def problems(*families):
    return [c.problem for c in T.fixed_set() if not families or c.family in families]


def both_params(oracle, **kw):
    pp, op = pkg().default_poa_params(), oracle.default_poa_params()
    for p_ in (pp, op):
        for k, v in kw.items():
            setattr(p_, k, v)
    return pp, op


@pytest.mark.parametrize("rule", [0, 1], ids=["longest-path", "first-out-edge"])
def test_fixed_set_under_both_remain_rules(once, ctx, rule):
    """several sources: poa_prepare counts only the first one under the first-out-edge rule; the best sink is picked over all"""
    _check_poa(once, ctx, problems(), *both_params(once, remain_rule=rule))


# the ids of test_poa_paths_the_library_can_fall_back_to (tests/test_gpu_parity.py)
SWITCHES = [{"VGA_POA_KERNEL": "t4"}, {"VGA_POA_KERNEL": "t5"}, {"VGA_POA_KERNEL": "t6"}, {"VGA_POA_KERNEL": "t6,generic"}, {"VGA_POA_KERNEL": "t7"},
            {"VGA_POA_KERNEL": "t7", "VGA_POA_T7_NT": "128", "VGA_POA_T7_WINDOW": "1024"}, {"VGA_POA_KERNEL": "unpacked"},
            {"VGA_POA_KERNEL": "generic"}, {"VGA_POA_ARENAS": "0"}, {"VGA_POA_ARENAS": "0", "VGA_POA_SLOTS": "1"}, {"VGA_POA_TB": "wave"},
            {"VGA_POA_TEXT": "host"}, {"VGA_POA_WINDOW": "256"}, {"VGA_POA_NT": "1024"}, {"VGA_POOL_BYTES": "300000000", "VGA_POA_SUB": "7"}]


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_fixed_set_under_the_kernel_switches(once, ctx, monkeypatch, env):
    """every DP kernel (k_poa_dp_t4 / _t5 / _t6 / _t7, k_poa_dp_lds as `unpacked`), the traceback kernel of its own, the classic
    pool, a 256-column LDS window (a multi-predecessor row on the HBM detour), 1 024 threads, tiny sub-batches in a small pool.
    VGA_POA_KERNEL=unpacked refuses queries beyond ~22 kbp; the longest query of the set has a few hundred bases, so no problem
    is left out under any configuration.  Two things keep the specialised kernels from most of the set as it stands: a launch
    whose width estimates stay below 1 000 columns is k_poa_dp_t6's whatever VGA_POA_KERNEL=t7 asks for, and k_poa_dp_t6 hands a
    problem back to k_poa_dp_t5 when its ring of fixed 6 192-byte slots does not fit the state region, which is sized by the
    launch's longest query (poa_state_size: 64 KiB for queries of a few hundred bases, i.e. edges of at most 9 nodes -- fans of
    17 arms and more go back).  So the t6 and t7 configurations get the problems of poa_topologies.wide_estimate_cases on top
    (1 230-base queries, estimates beyond 1 000 columns): the launch trace then shows k_poa_dp_t7 (256 threads) taking the
    whole batch and k_poa_dp_t6 and k_poa_dp_t7 (128 threads, 1 024 columns) all of it but the six added problems, whose rows on
    the long arm outgrow their windows -- fans of 255 arms included."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    wide = [c.problem for c in T.wide_estimate_cases()] if env.get("VGA_POA_KERNEL", "")[:2] in ("t6", "t7") else []
    _check_poa(once, ctx, problems() + wide)


@pytest.mark.parametrize("kw", [dict(gap_open1=6, gap_ext1=3, gap_open2=200, gap_ext2=1), dict(gap_open1=31, gap_ext1=33, gap_open2=24, gap_ext2=1),
                                dict(match=1, mismatch=3, gap_open1=2, gap_ext1=2, gap_open2=10, gap_ext2=1, wb=3, wf=0.05),
                                dict(match=1, mismatch=3, gap_open1=2, gap_ext1=2, gap_open2=10, gap_ext2=1, wb=-1), dict(wb=-1)],
                         ids=["k_poa_dp_lds", "k_poa_dp_t4", "narrow-band", "unbanded", "default-unbanded"])
def test_fans_and_far_edges_under_other_penalty_families(once, ctx, kw):
    """gap penalties that need 2-byte deltas are k_poa_dp_lds's, a first piece of open + extend = 64 is k_poa_dp_t4's: reached
    by the choice of family, not by a switch"""
    _check_poa(once, ctx, problems("fan", "reach"), *both_params(once, **kw))


def test_in_degree_255_is_served_and_256_is_refused(once, ctx):
    ok = [T.fan_limit_problem(255), T.fan_limit_problem(17)]
    _check_poa(once, ctx, ok)
    with pytest.raises(pkg().VgaError) as e:
        ctx.poa_batch([ok[1], T.fan_limit_problem(256)])
    assert e.value.code == -1 and "in-degree > 255" in str(e.value)
    _check_poa(once, ctx, ok)  # the context is as good as before


# ---------------------------------------------------------------- through vga_align_batch
@pytest.fixture(scope="module")
def bubbles(oracle):
    G = T.align_graph()
    return G, oracle.Index(oracle.Graph.from_nodes_edges(G.nodes, G.edges), 11)


def entries_of_reads(oracle, ix, G, gaf):
    """from the oracle alone: for every read, (position in the predecessor list, in-degree) of each join its path enters -- the
    list is that of the subgraph the read was aligned to (og_find_nodes_edges_for_abpoa) -- and whether it took the far edge"""
    entries, far = [], []
    for r, ln in zip(G.reads, gaf.splitlines()):
        path = [int(x) for x in ln.split("\t")[5].replace("<", ">").split(">")[1:]]
        _, cs, arr = oracle.chain_anchors(ix, r.seq, keep_raw=True)
        sg, _ = oracle.subgraph_for_chain(ix, cs, 0, len(r.seq))
        oracle.lib().og_chain_set_free(C.byref(cs))
        oracle.lib().og_free(arr)
        local = {h >> 1: i for i, h in enumerate(sg.range_handles)}
        preds = T.pred_lists(len(sg.nodes), sg.edges)
        for a, b in zip(path, path[1:]):
            if len(preds[local[b]]) > 1:
                entries.append((preds[local[b]].index(local[a]), len(preds[local[b]])))
        far.append((G.far_edge[0], G.far_edge[1]) in zip(path, path[1:]) and local[G.far_edge[1]] - local[G.far_edge[0]] > T.RING_SPAN)
    return entries, far


@pytest.mark.parametrize("rule", [0, 1], ids=["longest-path", "first-out-edge"])
def test_align_through_wide_bubbles_and_a_far_edge(oracle, ctx, bubbles, monkeypatch, rule):
    """a 40-allele bubble, a 9-allele bubble and a deletion edge that skips 40 nodes in a graph of its own: the node tables
    come from k_sg_emit (its in-degree and ring-span logic) and, with VGA_SUBGRAPH=host, from the host threads"""
    G, ix = bubbles
    upload_oracle_index(ctx, ix)
    dev = _check_align(oracle, ctx, ix, G.reads, remain_rule=rule)
    monkeypatch.setenv("VGA_SUBGRAPH", "host")
    host = _check_align(oracle, ctx, ix, G.reads, remain_rule=rule)
    monkeypatch.delenv("VGA_SUBGRAPH")
    assert dev.cigar == host.cigar and dev.path_handles.tolist() == host.path_handles.tolist() and dev.poa_cells == host.poa_cells
    assert int(dev.aligned.sum()) == len(G.reads)
    omp = oracle.default_map_params()
    omp.poa.remain_rule = rule
    _, gaf, _ = oracle.map_reads(ix, [r.name for r in G.reads], [r.seq for r in G.reads], omp)
    entries, far = entries_of_reads(oracle, ix, G, gaf)
    assert any(pos >= 4 for pos, _ in entries) and any(pos == deg - 1 and deg == 40 for pos, deg in entries), entries
    assert any(far) and not all(far)


def test_coverage_of_wide_bubbles_and_a_far_edge(oracle, ctx, bubbles):
    """k_cov_runs and k_poa_text branch on a row's number of predecessors: the tables of the same batch against the reference
    walker over the oracle's alignments"""
    G, ix = bubbles
    seqs = [r.seq for r in G.reads]
    want = walker(oracle, ix, seqs)
    assert want[3] == len(seqs)
    upload_oracle_index(ctx, ix)
    ctx.coverage_begin()
    try:
        b = ctx.batch(seqs)
        b.align(b.map())
        b.close()
        same(ctx.coverage(), want, "bubbles of 40 and 9 alleles")
    finally:
        ctx.coverage_end()


def test_align_refuses_a_bubble_of_256_alleles(oracle, ctx, bubbles, monkeypatch):
    """the subgraph of a read whose chain spans the bubble holds all 256 alleles (find_range_chain takes every node between the
    chain's ends), so the join has 256 predecessors there: vga_align_batch refuses the call like vga_poa_batch does, from the
    device subgraph builder and from the host threads, and the context goes on to serve the graph of 40 alleles"""
    G = T.align_graph(wide=256)
    ix = oracle.Index(oracle.Graph.from_nodes_edges(G.nodes, G.edges), 11)
    upload_oracle_index(ctx, ix)
    b = ctx.batch([r.seq for r in G.reads[:4]])
    mo = b.map()
    for route in (None, "host"):
        if route:
            monkeypatch.setenv("VGA_SUBGRAPH", route)
        with pytest.raises(pkg().VgaError) as e:
            b.align(mo)
        assert e.value.code == -1 and "in-degree > 255" in str(e.value), route
    monkeypatch.delenv("VGA_SUBGRAPH")
    b.close()
    G40, ix40 = bubbles
    upload_oracle_index(ctx, ix40)
    _check_align(oracle, ctx, ix40, G40.reads[:4])
