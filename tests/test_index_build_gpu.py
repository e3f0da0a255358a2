"""vga_index_build_kmers (csrc/vga_index.hip): the k-mer half of Index::build on the MI355X.  In every case the GPU-built
arrays equal both the C++ host builder's and the oracle's, field for field, through the C ABI and through
HostIndex.build_from_gfa(ctx=...); the CLI's `vgaligner index --device 0` writes the host's .idx byte for byte; the
context is left loaded exactly as vga_index_upload of the host index leaves it."""
import filecmp
import os
import subprocess

import numpy as np
import pytest

from helpers import DATA, ROOT, oracle_index_arrays, pkg

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
TEST_GFA = os.path.join(DATA, "test.gfa")
KMER_FIELDS = ("kmer_keys", "kmer_starts", "kmer_pos_table")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


def _gfa(tmp_path, name, nodes, links):
    """links: (from, from_orient, to, to_orient) with orient '+' / '-'"""
    p = tmp_path / f"{name}.gfa"
    lines = ["H\tVN:Z:1.0"] + [f"S\t{i}\t{s}" for i, s in nodes] + [f"L\t{a}\t{ao}\t{b}\t{bo}\t0M" for a, ao, b, bo in links]
    p.write_text("\n".join(lines) + "\n")
    return str(p)


def _fwd(edges):
    return [(a, "+", b, "+") for a, b in edges]


def _same(a, b, what):
    for f in KMER_FIELDS:
        x, y = a[f], b[f]
        if isinstance(x, np.ndarray):
            assert len(x) == len(y), (what, f, len(x), len(y))
            if x.dtype.names:
                for n in x.dtype.names:
                    assert np.array_equal(x[n], y[n]), (what, f, n)
            else:
                assert np.array_equal(np.asarray(x, np.uint64), np.asarray(y, np.uint64)), (what, f)
        else:
            assert bytes(x) == bytes(y), (what, f)


def _abi_build(ctx, host, k=None, furc=100, deg=100):
    """the graph half of a host index through vga_index_build_kmers; returns the k-mer arrays"""
    b = pkg().binding
    a = host.arrays()
    d = b.graph_desc(k or a["k"], a["seq_fwd"], a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    ctx.index_build_kmers(d, furc, deg)
    try:
        return b.kmer_arrays(d)
    finally:
        b.index_kmers_free(d)


def check(ctx, oracle, path, k, furc=100, deg=100):
    """GPU == host == oracle for one graph; returns the GPU arrays"""
    HostIndex = pkg().HostIndex
    host = HostIndex.build_from_gfa(path, k, furc, deg).arrays()
    want = oracle_index_arrays(oracle.Index(oracle.Graph.from_gfa(path), k, furc, deg))
    _same(host, want, "host vs oracle")
    dev = HostIndex.build_from_gfa(path, k, furc, deg, ctx=ctx).arrays()
    for f in ("seq_fwd", "node_seq_idx", "node_edge_idx", "node_edges_to", "edges"):
        assert np.array_equal(np.asarray(dev[f]), np.asarray(host[f])) if isinstance(host[f], np.ndarray) else dev[f] == host[f], f
    _same(dev, host, f"gpu vs host {os.path.basename(path)} k={k}")
    _same(dev, want, f"gpu vs oracle {os.path.basename(path)} k={k}")
    _same(_abi_build(ctx, HostIndex.build_from_gfa(path, k, furc, deg), furc=furc, deg=deg), host, "C ABI vs host")
    return dev


def positions(a, kmer):
    k = len(kmer)
    keys = [a["kmer_keys"][i:i + k] for i in range(0, len(a["kmer_keys"]), k)]
    s = int(a["kmer_starts"][keys.index(kmer.encode())])
    out = []
    while int(a["kmer_pos_table"][s]["start"]) != 2**64 - 1:
        t = a["kmer_pos_table"][s]
        out.append((int(t["start_orient"]), int(t["start"]), int(t["end_orient"]), int(t["end"])))
        s += 1
    return out


SIMPLE = [(1, "A"), (2, "CT"), (3, "GA"), (4, "GCA")], [(1, 2), (1, 3), (2, 4), (3, 4)]


# ---------------------------------------------------------------- the reference's graphs
@pytest.mark.parametrize("k", [3, 5, 6])
def test_simple_graph(ctx, oracle, tmp_path, k):
    """src/index.rs:654-678 simple graph"""
    a = check(ctx, oracle, _gfa(tmp_path, "simple", SIMPLE[0], _fwd(SIMPLE[1])), k)
    if k == 3:
        assert positions(a, "ACT")[0] == (0, 0, 0, 3)


def test_simple_path(ctx, oracle, tmp_path):
    """src/index.rs:843-890"""
    check(ctx, oracle, _gfa(tmp_path, "path", [(1, "ACG"), (2, "TTT"), (3, "CA")], _fwd([(1, 2), (2, 3)])), 3)


def test_diamond(ctx, oracle, tmp_path):
    """the second graph of src/index.rs:1246-1258 test_compare_sequential_parallel_graphkmer"""
    check(ctx, oracle, _gfa(tmp_path, "diamond", [(1, "GAT"), (2, "T"), (3, "A"), (4, "CA")], _fwd([(1, 2), (1, 3), (2, 4), (3, 4)])), 3)


def test_multinode_kmers(ctx, oracle, tmp_path):
    """src/index.rs:1669-1732: spans asserted on the GPU-built table"""
    a = check(ctx, oracle, _gfa(tmp_path, "simple", SIMPLE[0], _fwd(SIMPLE[1])), 5)
    assert positions(a, "ACTGC") and positions(a, "CTGCA")
    g2 = [(1, "ACG"), (2, "C"), (3, "G"), (4, "TTTTT")], [(1, 2), (1, 3), (2, 4), (3, 4)]
    a = check(ctx, oracle, _gfa(tmp_path, "g2", g2[0], _fwd(g2[1])), 5)
    assert (positions(a, "ACGGT")[0][1], positions(a, "ACGGT")[0][3]) == (0, 6)
    assert (positions(a, "GCTTT")[0][1], positions(a, "GCTTT")[0][3]) == (2, 8)
    assert (positions(a, "CTTTT")[0][1], positions(a, "CTTTT")[0][3]) == (3, 9)
    g3 = ([(1, "ACG"), (2, "C"), (3, "G"), (4, "TTTTT"), (5, "TA"), (6, "CG"), (7, "TTT")],
          [(1, 2), (1, 3), (2, 4), (3, 4), (4, 5), (4, 6), (5, 7), (6, 7)])
    a = check(ctx, oracle, _gfa(tmp_path, "g3", g3[0], _fwd(g3[1])), 5)
    assert (positions(a, "TTCGT")[0][1], positions(a, "TTCGT")[0][3]) == (8, 15)


def test_single_node(ctx, oracle, tmp_path):
    check(ctx, oracle, _gfa(tmp_path, "one", [(1, "ACGTTGCAAGT")], []), 4)


# ---------------------------------------------------------------- in-tree and generated graphs
@pytest.mark.parametrize("path,k", [(TEST_GFA, 3), (TEST_GFA, 11), (DRB1, 7), (DRB1, 11), (DRB1, 15)])
def test_in_tree_graphs(ctx, oracle, path, k):
    check(ctx, oracle, path, k)


def test_config4(ctx, oracle, config4_gfa):
    check(ctx, oracle, config4_gfa, 11)


@pytest.mark.parametrize("k", [11, 13, 15])
def test_config5_60k(ctx, oracle, config5_small_gfa, k):
    check(ctx, oracle, config5_small_gfa, k)


def test_config5_1mbp(ctx, oracle, tmp_path):
    path = str(tmp_path / "syn1m.gfa")
    pkg().readsim.synth_pangenome(path, 1_000_000, seed=77)
    check(ctx, oracle, path, 11)


# ---------------------------------------------------------------- the rules, graph by graph
def test_n_in_start_node(ctx, oracle, tmp_path):
    nodes = [(1, "ACGTA"), (2, "CCNAG"), (3, "GTTAC"), (4, "TGCA")]
    a = check(ctx, oracle, _gfa(tmp_path, "n1", nodes, _fwd([(1, 2), (2, 3), (3, 4), (1, 3)])), 4)
    assert a["kmer_keys"]


def test_n_reached_only_through_the_dfs(ctx, oracle, tmp_path):
    """node 2's k-mers meet node 3's N only when the DFS extends them into node 3: 2+ is discarded, 1+ is not
    (its extensions stop within k - 1 bases, before node 3)"""
    nodes = [(1, "ACGTACG"), (2, "TTGCA"), (3, "NGATCA"), (4, "CATTAG")]
    check(ctx, oracle, _gfa(tmp_path, "n3", nodes, _fwd([(1, 2), (2, 3), (3, 4), (1, 4)])), 5)


@pytest.mark.parametrize("furc,deg", [(1, 1), (1, 2), (2, 1), (2, 2)])
def test_furcations_and_degree(ctx, oracle, furc, deg):
    check(ctx, oracle, DRB1, 11, furc, deg)


def test_start_handle_above_max_degree(ctx, oracle, tmp_path):
    nodes = [(1, "ACG"), (2, "T"), (3, "G"), (4, "C"), (5, "AAT")]
    edges = [(1, 2), (1, 3), (1, 4), (2, 5), (3, 5), (4, 5)]
    for deg in (2, 3, 4):
        check(ctx, oracle, _gfa(tmp_path, f"deg{deg}", nodes, _fwd(edges)), 4, 100, deg)


def test_identical_bubble_arms_are_deduplicated(ctx, oracle, tmp_path):
    """1:AC -> {2:G, 3:G} -> 4:TA: CGT from offset 1 of node 1 through either arm is the same record (same ends, forks 1)"""
    nodes = [(1, "AC"), (2, "G"), (3, "G"), (4, "TA")]
    a = check(ctx, oracle, _gfa(tmp_path, "bubble", nodes, _fwd([(1, 2), (1, 3), (2, 4), (3, 4)])), 3)
    # forward: emitted once per arm, kept once; reverse: from 2- and from 3-, two start handles, both kept
    assert positions(a, "CGT") == [(0, 1, 0, 5), (1, 2, 1, 6), (1, 3, 1, 6)]


def test_reverse_link_and_self_loop(ctx, oracle, tmp_path):
    nodes = [(1, "ACGTT"), (2, "GGCA"), (3, "TTAG"), (4, "CAGT")]
    links = [(1, "+", 2, "+"), (2, "+", 3, "-"), (3, "-", 4, "+"), (4, "+", 4, "+"), (1, "+", 3, "+"), (2, "-", 1, "-")]
    check(ctx, oracle, _gfa(tmp_path, "rev", nodes, links), 4)
    check(ctx, oracle, _gfa(tmp_path, "rev", nodes, links), 7)


def test_chain_of_bubbles(ctx, oracle, tmp_path):
    """14 single-base bubbles in a row at k = 15: 2^14 paths from the first node"""
    nodes, edges = [(1, "A")], []
    nid = 1
    for i in range(14):
        a, b, j = nid + 1, nid + 2, nid + 3
        nodes += [(a, "C"), (b, "G"), (j, "T")]
        edges += [(nid, a), (nid, b), (a, j), (b, j)]
        nid = j
    check(ctx, oracle, _gfa(tmp_path, "bubbles", nodes, _fwd(edges)), 15)


# ---------------------------------------------------------------- the CLI writes the same file
@pytest.mark.parametrize("which", ["drb1", "config4"])
def test_cli_device_writes_the_host_idx(tmp_path, config4_gfa, which):
    pkg()
    exe = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
    gfa = DRB1 if which == "drb1" else config4_gfa
    outs = []
    for extra, name in (([], "host"), (["--device", "0"], "gpu")):
        r = subprocess.run([exe, "index", "-i", gfa, "-k", "11", "-o", str(tmp_path / name)] + extra, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr
        outs.append(r.stderr)
    assert outs[0] == outs[1]
    assert filecmp.cmp(tmp_path / "host.idx", tmp_path / "gpu.idx", shallow=False)


# ---------------------------------------------------------------- the context is loaded
def _arrays_of(obj):
    return {k: v for k, v in vars(obj).items() if isinstance(v, (np.ndarray, list, bytes, int))}


def _same_results(x, y, what):
    a, b = _arrays_of(x), _arrays_of(y)
    assert a.keys() == b.keys(), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def test_built_context_maps_and_aligns_like_an_uploaded_one(ctx):
    p = pkg()
    host = p.HostIndex.build_from_gfa(DRB1, 11)
    up = p.Context(0)
    try:
        host.upload(up)
        p.HostIndex.build_from_gfa(DRB1, 11, ctx=ctx)
        rs = p.readsim
        sets = {"config2": [r.seq for r in rs.config2_reads(DRB1, 300)], "config3": [r.seq for r in rs.config3_reads(DRB1, 200)]}
        for name, seqs in sets.items():
            for only_forward in (1, 0):
                mp = p.binding.default_map_params()
                mp.only_forward = only_forward
                outs = []
                for c in (ctx, up):
                    b = c.batch(seqs)
                    m = b.map(mp)
                    al = b.align(m) if only_forward else None
                    outs.append((m, al))
                _same_results(outs[0][0], outs[1][0], f"map {name} only_forward={only_forward}")
                assert [outs[0][0].chains_of(r) for r in range(len(seqs))] == [outs[1][0].chains_of(r) for r in range(len(seqs))]
                if only_forward:
                    _same_results(outs[0][1], outs[1][1], f"align {name}")
    finally:
        up.close()


# ---------------------------------------------------------------- refusals and lifetime
def _map_code(ctx):
    with pytest.raises(pkg().binding.VgaError) as e:
        ctx.batch(["ACGTACGTACGTACGTACGT"]).map()
    return e.value.code


def test_refusals_leave_no_index(ctx, tmp_path):
    p = pkg()
    b = p.binding
    host = p.HostIndex.build_from_gfa(DRB1, 11)
    p.HostIndex.build_from_gfa(DRB1, 11, ctx=ctx)  # a loaded context first: each refusal must unload it
    with pytest.raises(b.VgaError) as e:
        _abi_build(ctx, host, k=16)
    assert e.value.code == -4
    assert _map_code(ctx) == -5
    a = host.arrays()
    low = a["seq_fwd"][:10] + a["seq_fwd"][10:11].lower() + a["seq_fwd"][11:]
    d = b.graph_desc(11, low, a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    p.HostIndex.build_from_gfa(DRB1, 11, ctx=ctx)
    with pytest.raises(b.VgaError) as e:
        ctx.index_build_kmers(d)
    assert e.value.code == -4 and "A/C/G/T/N" in str(e.value)
    assert _map_code(ctx) == -5
    tiny = p.HostIndex.build_from_gfa(_gfa(tmp_path, "tiny", [(1, "ACG"), (2, "T")], _fwd([(1, 2)])), 3)
    p.HostIndex.build_from_gfa(DRB1, 11, ctx=ctx)
    with pytest.raises(b.VgaError) as e:
        _abi_build(ctx, tiny, k=5)
    assert "the graph has no k-mer of this length" in str(e.value)
    assert _map_code(ctx) == -5
    with pytest.raises(p.hostlib.HostError, match="no k-mer of this length"):
        p.HostIndex.build_from_gfa(_gfa(tmp_path, "tiny", [(1, "ACG"), (2, "T")], _fwd([(1, 2)])), 5, ctx=ctx)


def test_twice_identical_and_free_zeroes(ctx):
    p = pkg()
    b = p.binding
    host = p.HostIndex.build_from_gfa(DRB1, 13)
    _same(_abi_build(ctx, host), _abi_build(ctx, host), "two builds")
    a = host.arrays()
    d = b.graph_desc(13, a["seq_fwd"], a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    ctx.index_build_kmers(d)
    assert d.n_kmers and d.n_kmer_pos and d.kmer_keys and d.kmer_starts and d.kmer_pos_table
    names = [t["name"] for t in ctx.kernel_times()]
    for n in ("k_ix_count", "k_ix_emit", "k_ix_sort_kmer", "k_ix_dedup", "k_ix_sort_pos", "k_ix_groups", "k_ix_probe"):
        assert n in names, names
    b.index_kmers_free(d)
    assert (d.n_kmers, d.n_kmer_pos) == (0, 0)
    assert not d.kmer_keys and not d.kmer_starts and not d.kmer_pos_table
