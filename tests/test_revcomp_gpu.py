"""k_revcomp_reads (csrc/vga_strand.hip) and vga_batch_revcomp_host, read back through the seam vga_batch_strands
(Batch.strands): the seeded batches of tests/revcomp_cases.py against the plain reference, byte for byte; the forward half
untouched; the two routes equal; and the seam before and after a map call of the same batch."""
import ctypes as C
import os

import numpy as np
import pytest

import revcomp_cases as rcc
from helpers import DATA, pkg, upload_oracle_index
from test_both_strands_gpu import MAP_FIELDS

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """{batch name: (forward half, reverse half)}"""
    return {b.name: (b"".join(b.reads), b"".join(rcc.reverse_complement(r) for r in b.reads)) for b in rcc.batches()}


def assert_reverse_half(batch, got, want, route):
    assert len(got) == len(want), "%s, %s: %d bytes, %d expected" % (batch.name, route, len(got), len(want))
    if got == want:
        return
    at = next(i for i in range(len(want)) if got[i] != want[i])
    off = rcc.offsets(batch.reads)
    r = next(i for i in range(len(batch.reads)) if off[i] <= at < off[i + 1])
    t = rcc.tile_of(batch.reads, r, at - off[r])
    raise AssertionError("%s, %s: read %d (%d bytes at offset %d), byte %d is %r, expected %r; its tile starts at byte %d with (s0 & 3, d0 & 3, n) = (%d, %d, %d); "
                         "%d bytes of the half differ" % (batch.name, route, r, len(batch.reads[r]), off[r], at - off[r], got[at:at + 1], want[at:at + 1],
                                                          t.i0, t.s0 & 3, t.d0 & 3, t.n, sum(a != b for a, b in zip(got, want))))


@pytest.mark.parametrize("batch", rcc.batches(), ids=lambda b: b.name)
def test_seeded_batches(ctx, expected, batch):
    fwd, rev = expected[batch.name]
    b = ctx.batch(list(batch.reads))
    dev = b.strands()
    assert_reverse_half(batch, dev[1], rev, "device")
    assert dev[0] == fwd, "the forward half after the copy into the larger allocation"
    host = b.strands(from_host=True)
    assert_reverse_half(batch, host[1], rev, "host")
    assert host[0] == fwd and host == dev
    assert b.strands() == dev and b.strands(from_host=True) == host, "a second call"
    # the host's half first, on a batch of its own
    b2 = ctx.batch(list(batch.reads))
    assert b2.strands(from_host=True) == dev and b2.strands() == dev
    b.close()
    b2.close()


def test_the_kernel_ran(ctx):
    b = ctx.batch([b"ACGTN" * 300])
    b.strands()
    assert [k["launches"] for k in ctx.kernel_times() if k["name"] == "revcomp_reads"] == [1]


def test_refusals(ctx):
    p = pkg()
    L = ctx.L
    assert L.vga_batch_strands(None, 0, None, None) == -1  # VGA_ERR_ARG
    other = p.Context(0)
    b = other.batch(["ACGT"])
    other.close()
    assert L.vga_batch_strands(b.h, 0, None, None) == -1  # (its context is gone)
    b.close()
    # either half may be left out
    b = ctx.batch(["AACGT", "", "acgu"])
    buf = C.create_string_buffer(9)
    assert L.vga_batch_strands(b.h, 0, None, buf) == 0 and buf.raw == b"ACGTTacgt"
    assert L.vga_batch_strands(b.h, 1, buf, None) == 0 and buf.raw == b"AACGTacgu"
    assert L.vga_batch_strands(b.h, 0, None, None) == 0


# ---------------------------------------------------------------- the seam and the map call in either order
@pytest.fixture(scope="module")
def drb1_case(oracle, ctx):
    p = pkg()
    upload_oracle_index(ctx, oracle.Index(oracle.Graph.from_gfa(DRB1), 11))
    reads = p.readsim.simulate_reads(DRB1, 6, 1500, 0.03, 0.03, 0.04, seed=61)
    seqs = [p.readsim.reverse_complement(r.seq) for r in reads] + [reads[0].seq, "ACGTT"]
    halves = ("".join(seqs).encode(), b"".join(rcc.reverse_complement(s.encode()) for s in seqs))
    return seqs, halves


def both_params():
    p = pkg()
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    return mp


def same_fields(a, b, fields):
    for name in fields:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_seam_and_map_in_either_order(ctx, drb1_case):
    seqs, halves = drb1_case
    b1 = ctx.batch(seqs)
    first = b1.strands()
    m1 = b1.map(both_params())
    b2 = ctx.batch(seqs)
    m2 = b2.map(both_params())
    after = b2.strands()
    assert first == halves and after == halves and b1.strands() == halves
    assert m1.strand.tolist() == m2.strand.tolist() == [1] * 6 + [0, 0]
    same_fields(m1, m2, MAP_FIELDS + ("anchor_id", "max_chain_score", "best_pred_id"))
    assert m1.n_anchors > 1000
    # the host's half beside them changes nothing either
    assert b1.strands(from_host=True) == halves
    same_fields(b1.map(both_params()), m1, MAP_FIELDS + ("strand",))


def test_forward_map_after_the_seam(ctx, drb1_case):
    seqs, halves = drb1_case
    fresh = ctx.batch(seqs).map()
    b = ctx.batch(seqs)
    assert b.strands() == halves and b.strands(from_host=True) == halves
    m = b.map()
    assert m.strand is None
    same_fields(m, fresh, MAP_FIELDS + ("anchor_id", "max_chain_score", "best_pred_id"))
    assert m.n_hits == fresh.n_hits
