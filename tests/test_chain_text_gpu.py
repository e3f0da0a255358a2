"""k_gaf_chain_len / k_gaf_chain_write (csrc/vga_gaf.hip) through Context.chain_paths_text: the planted cases of
tests/chain_text_cases.py on the digits graph against the plain reference, chain by chain and byte for byte; real map results on
DRB1 against column 6 of the oracle's chains GAF; the call beside an alignment on the same context; its refusals.  The 10-digit
branch of gaf_digits needs a position of 10^9 or more, a graph of 1 GB: it is not covered."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import chain_text_cases as ctc
from helpers import DATA, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")


@pytest.fixture(scope="module")
def ctx():
    """one context holding the digits graph, uploaded once for the module"""
    c = pkg().Context(0)
    t0 = time.perf_counter()
    ctc.digits_graph().upload(c)
    print("digits graph: %d bases, %d nodes, uploaded in %.2f s" % (ctc.digits_graph().seq_length, ctc.digits_graph().n_nodes, time.perf_counter() - t0))
    yield c
    c.close()


@pytest.fixture(scope="module")
def references():
    return {c.name: ctc.reference(c) for c in ctc.all_cases()}


def check(ctx, case, want):
    got = ctx.chain_paths_text(case.result())
    assert got == want, ctc.describe_first_difference(case, got, want)
    return got


@pytest.mark.parametrize("case", ctc.all_cases(), ids=repr)
def test_planted_cases(ctx, references, case):
    want = references[case.name]
    check(ctx, case, want)
    # the offsets themselves: the total is the sum of the chains, and every chain starts where the one before ended
    p = pkg()
    out = C.POINTER(p.binding.ChainText)()
    ctx._check(ctx.L.vga_chain_paths_text(ctx.h, case.result()._ptr, C.byref(out)))
    try:
        off = [int(out.contents.text_off[i]) for i in range(case.n_chains + 1)]
        assert int(out.contents.n_chains) == case.n_chains
    finally:
        ctx.L.vga_chain_text_free(out)
    assert off[0] == 0 and off[-1] == sum(len(t) for t in want) and np.diff(off).tolist() == [len(t) for t in want]
    if case.name == "only-placeholders":
        assert off == [0] * (case.n_chains + 1)


def test_workspace_is_reused_from_call_to_call(ctx, references):
    """grow-only buffers: the largest case, the smallest, the largest again, each right"""
    for name in ("chains-40000", "chains-1", "chains-40000", "text-lengths", "only-placeholders", "chains-1"):
        check(ctx, ctc.case(name), references[name])


# ---------------------------------------------------------------- real map results
@pytest.fixture(scope="module")
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


@pytest.fixture(scope="module")
def drb1_ctx(drb1):
    c = pkg().Context(0)
    upload_oracle_index(c, drb1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1_reads():
    """plain reads, reads with two chains (as test_best_of_two_candidates builds them) and a read that is too short to anchor"""
    src = pkg().readsim.simulate_reads(DRB1, 6, 700, 0.02, 0.02, 0.02, seed=23)
    return [r.seq for r in src] + [r.seq[:500] + r.seq[:500] for r in src] + ["ACGTTGCA", src[0].seq[:300] * 3]


def oracle_column(oracle, ix, seqs):
    mp = oracle.default_map_params(also_align=False)
    lines = oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, mp)[0].splitlines()
    return [b"" if f == "*" else f.encode() for f in (ln.split("\t")[5] for ln in lines)]


def test_drb1_map_results(oracle, drb1, drb1_ctx, drb1_reads):
    p = pkg()
    want = oracle_column(oracle, drb1, drb1_reads)
    b = drb1_ctx.batch(drb1_reads)
    mo = b.map()
    assert max(len(mo.chains_of(r)) for r in range(len(drb1_reads))) >= 2 and mo.chain_placeholder.any() and b"" in want
    assert drb1_ctx.chain_paths_text(mo) == want
    mp = p.default_map_params()
    mp.emit_dp = 0
    m0 = b.map(mp)
    assert m0.anchor_id is None and drb1_ctx.chain_paths_text(m0) == want


def test_drb1_both_strands(oracle, drb1, drb1_ctx, drb1_reads):
    p = pkg()
    rc = p.readsim.reverse_complement
    given = [rc(s) if i % 2 == 0 else s for i, s in enumerate(drb1_reads)]
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    mo = drb1_ctx.batch(given).map(mp)
    strand = mo.strand.tolist()
    assert 3 <= sum(strand) < len(given)
    chosen = [rc(s) if st else s for s, st in zip(given, strand)]
    assert drb1_ctx.chain_paths_text(mo) == oracle_column(oracle, drb1, chosen)


def test_beside_the_alignment_on_one_context(drb1_ctx):
    """the one concurrent use the header documents and the host driver makes: a thread in vga_chain_paths_text while another
    is in vga_align_batch on the same context"""
    reads = pkg().readsim.simulate_reads(DRB1, 48, 1500, 0.03, 0.03, 0.04, seed=41)
    b = drb1_ctx.batch([r.seq for r in reads])
    mo = b.map()
    text, al = drb1_ctx.chain_paths_text(mo), b.align(mo)
    box = {}

    def side():
        try:
            box["text"] = drb1_ctx.chain_paths_text(mo)
        except Exception as e:  # (reported by the main thread)
            box["error"] = e

    th = threading.Thread(target=side)
    th.start()
    al2 = b.align(mo)
    th.join()
    assert "error" not in box, box.get("error")
    assert box["text"] == text and sum(map(len, text)) > 100000
    assert al2.cigar == al.cigar and al2.cs == al.cs and al2.aligned.tolist() == al.aligned.tolist()
    assert al2.path_handles.tolist() == al.path_handles.tolist() and int(al.aligned.sum()) >= 40


def test_refusals(ctx):
    p = pkg()
    L = ctx.L
    m = ctc.case("chains-1").result()
    bare = p.Context(0)
    try:
        with pytest.raises(p.VgaError) as e:
            bare.chain_paths_text(m)
        assert e.value.code == -5  # VGA_ERR_NO_INDEX
    finally:
        bare.close()
    out = C.POINTER(p.binding.ChainText)()
    assert L.vga_chain_paths_text(None, m._ptr, C.byref(out)) == -1  # VGA_ERR_ARG
    assert L.vga_chain_paths_text(ctx.h, None, C.byref(out)) == -1
    assert L.vga_chain_paths_text(ctx.h, m._ptr, None) == -1
    assert not out
    check(ctx, ctc.case("chains-1"), ctc.reference(ctc.case("chains-1")))
