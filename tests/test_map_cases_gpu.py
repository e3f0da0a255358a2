"""k_kmer_probe / k_anchor_sort / k_chain4 / k_strand_pick (csrc/vga_map.hip) on the cases of tests/map_cases.py -- score ties at
most steps, anchor counts around the 64-anchor load block, gaps of exactly max_gap with the gap-cost table in LDS and in HBM,
graph lengths at the edges of the sort's pass count, reads on both sides of the integer-argmax threshold in one launch,
several chains on one maximum, strand ties -- held to the oracle bit for bit with helpers.compare_map, and through
vga_align_batch where the order of tied chains decides what is aligned.  tests/test_map_cases_cpu.py shows from the oracle
alone that every case produces its condition."""
from collections import namedtuple

import numpy as np
import pytest

import map_cases as M
from helpers import compare_map, pkg, upload_oracle_index
from test_both_strands_gpu import check_map

pytestmark = pytest.mark.gpu

DP_FIELDS = ("anchor_off", "anchor_id", "query_begin", "target_begin", "target_end", "max_chain_score", "best_pred_id", "curr_max",
             "chain_off", "chain_placeholder", "chain_anchor_off", "chain_anchor_idx")
Read = namedtuple("Read", "name seq")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


class _OracleOnce:
    """the oracle with its indexes and chain_anchors results remembered: a read is chained once per parameter set, however
    many kernel configurations are held to it"""

    def __init__(self, oracle):
        self.o, self.indexes, self.seen = oracle, {}, {}

    def __getattr__(self, name):
        return getattr(self.o, name)

    def index(self, case):
        key = (tuple(case.nodes), case.k)
        if key not in self.indexes:
            self.indexes[key] = self.o.Index(self.o.Graph.from_nodes_edges(case.nodes, case.edges), case.k)
        return self.indexes[key]

    def chain_anchors(self, ix, s, bandwidth=50, max_gap=1000, min_anchors=3, only_forward=True):
        key = (id(ix), s, bandwidth, max_gap, min_anchors, only_forward)
        if key not in self.seen:
            self.seen[key] = (ix, self.o.chain_anchors(ix, s, bandwidth, max_gap, min_anchors, only_forward=only_forward))
        return self.seen[key][1]


@pytest.fixture(scope="module")
def once(oracle):
    return _OracleOnce(oracle)


def case(name):
    return next(c for c in M.all_cases() if c.name == name)


def names(*families):
    return [c.name for c in M.all_cases() if c.family in families]


def map_params(c):
    mp, p = pkg().default_map_params(), M.params_of(c)
    mp.bandwidth, mp.max_gap, mp.chain_min_n_anchors = p["bandwidth"], p["max_gap"], p["chain_min_n_anchors"]
    mp.only_forward, mp.strands = p["only_forward"], p["strands"]
    return mp


def map_and_compare(once, ctx, ix, c):
    p = M.params_of(c)
    b = ctx.batch(c.reads)
    mo = b.map(map_params(c))
    compare_map(once, ix, mo, c.reads, p["bandwidth"], p["max_gap"], p["chain_min_n_anchors"], bool(p["only_forward"]))
    return b, mo


def same_results(a, b):
    for f in DP_FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        assert np.array_equal(x, y), f


# ---------------------------------------------------------------- map parity
@pytest.mark.parametrize("name", names("repeat", "count", "argmax"))
def test_map_with_the_integer_and_the_f64_argmax(once, ctx, monkeypatch, name):
    """a. repeats: ties at most steps, the window's largest j wins; b. anchor counts on both sides of the 64-anchor blocks with
    windows of 1, 63 and 64; e. reads above and below key_anchors in the workgroups of one launch.  Then every read through the
    f64 reduction: the same bits"""
    c = case(name)
    ix = once.index(c)
    upload_oracle_index(ctx, ix)
    _, mi = map_and_compare(once, ctx, ix, c)
    monkeypatch.setenv("VGA_CHAIN_F64", "1")
    _, mf = map_and_compare(once, ctx, ix, c)
    same_results(mi, mf)


@pytest.mark.parametrize("name", names("gap", "equal"))
def test_map_gap_limits_and_equal_chains(once, ctx, name):
    """c. a jump of exactly max_gap reads the last entry of the gap-cost table, in LDS up to max_gap = 2047 and in HBM from 2048
    (32 MB at the largest max_gap), and one of max_gap + 1 is refused; f. several chains end on the same maximum"""
    c = case(name)
    ix = once.index(c)
    upload_oracle_index(ctx, ix)
    map_and_compare(once, ctx, ix, c)


def _fill_the_sort_buffers(ctx, c):
    """50 anchors in one read: both ping-pong buffers of k_anchor_sort hold a permutation up to where the case's one-anchor read
    comes to lie, whatever an earlier test left there"""
    ctx.batch([M.linear_sequence(c)[:60]]).map(map_params(c))


@pytest.mark.parametrize("name", names("sort"))
def test_map_sort_key_width(once, ctx, name):
    """d. 1, 2 and 3 radix passes and target_end == seq_length on the last k-mer; the one-anchor read between two others"""
    c = case(name)
    ix = once.index(c)
    upload_oracle_index(ctx, ix)
    _fill_the_sort_buffers(ctx, c)
    map_and_compare(once, ctx, ix, c)


@pytest.mark.parametrize("name", names("sort"))
def test_map_sort_key_width_on_a_device_built_index(once, ctx, tmp_path, name):
    """the same through vga_index_build_kmers: the pass count follows the seq_length the device build leaves in the context"""
    c = case(name)
    gfa = tmp_path / (name + ".gfa")
    gfa.write_text("\n".join(["H\tVN:Z:1.0"] + ["S\t%d\t%s" % ns for ns in c.nodes] + ["L\t%d\t+\t%d\t+\t0M" % e for e in c.edges]) + "\n")
    pkg().HostIndex.build_from_gfa(str(gfa), c.k, ctx=ctx)
    _fill_the_sort_buffers(ctx, c)
    map_and_compare(once, ctx, once.index(c), c)


# ---------------------------------------------------------------- strands
def test_strand_ties_keep_the_read_as_given(once, ctx):
    """g. S, rc(S) and a palindrome on S - spacer - rc(S): curr_max is bit-equal either way and k_strand_pick keeps '+'"""
    c = M.strand_case()
    ix = once.index(c)
    upload_oracle_index(ctx, ix)
    _, mo, chosen = check_map(once, ctx, ix, [Read("r%d" % i, s) for i, s in enumerate(c.reads)])
    assert mo.strand.tolist() == [0, 0, 0, 1]
    assert all(mo.strand[r] == 0 for r in M.STRAND_TIE_READS)
    assert chosen[:3] == c.reads[:3] and chosen[3] == M.rc(c.reads[3])


# ---------------------------------------------------------------- through vga_align_batch
@pytest.mark.parametrize("name", [n for n in names("repeat", "gap", "equal") if "-all-" not in n])
def test_align_what_the_tied_chains_select(once, ctx, name):
    """a, c, f: the first chain of a read is the one that is aligned, so the order of tied chains shows in the alignment"""
    c = case(name)
    p = M.params_of(c)
    ix = once.index(c)
    upload_oracle_index(ctx, ix)
    b, mo = map_and_compare(once, ctx, ix, c)
    al = b.align(mo)
    omp = once.default_map_params()
    omp.bandwidth, omp.max_gap, omp.chain_min_n_anchors = p["bandwidth"], p["max_gap"], p["chain_min_n_anchors"]
    _, ag, st = once.map_reads(ix, ["r%d" % i for i in range(len(c.reads))], c.reads, omp)
    lines = ag.splitlines()
    assert len(lines) == len(c.reads)
    for r, ln in enumerate(lines):
        f = ln.split("\t")
        if f[5] == "*":
            assert not al.aligned[r], f"read {r} aligned on the GPU only"
            continue
        assert al.aligned[r], f"read {r} aligned on the CPU only"
        hs = al.path_handles[int(al.path_off[r]):int(al.path_off[r + 1])].tolist()
        assert "".join((">" if not (h & 1) else "<") + str(h >> 1) for h in hs) == f[5], f"read {r}: node path"
        assert f[12] == "as:i:-30 " + al.cs[r] + ",cg:Z:" + al.cigar[r], f"read {r}: cs / CIGAR"
        assert (int(f[6]), int(f[7]), int(f[8]), int(f[10])) == (
            int(al.path_length[r]), int(al.path_start[r]), int(al.path_end[r]), int(al.block_length[r]))
    assert al.poa_cells == st["poa_cells"] and al.poa_rows == st["poa_rows"]
