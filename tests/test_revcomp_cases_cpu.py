"""tests/revcomp_cases.py without a GPU: the batches hold every start of a tile's source and destination inside a 32-bit word on
every kind of tile, the lengths and contents they are there for, and the reference equals the product's own Python reverse
complement on ASCII reads."""
import random

import revcomp_cases as rcc
from helpers import pkg


def test_table_is_the_rule():
    t = rcc.TABLE
    assert len(t) == 256 and bytes(t[c] for c in b"ACGTacgtUu") == b"TGCAtgcaAa"
    assert all(t[c] == ord("N") for c in range(256) if c not in b"ACGTacgtUu")
    assert rcc.reverse_complement(b"AACGTxu\x00\xff") == b"NNaNACGTT"


def test_reference_equals_readsim_on_ascii_reads():
    rs = pkg().readsim
    rng = random.Random(7)
    for n in (0, 1, 2, 63, 1024, 1500):
        for alphabet in ("ACGT", "ACGTacgtUuNnRYK-*. "):
            s = "".join(rng.choice(alphabet) for _ in range(n))
            assert rcc.reverse_complement(s.encode()) == rs.reverse_complement(s).encode()
    s = "".join(chr(c) for c in range(128))
    assert rcc.reverse_complement(s.encode()) == rs.reverse_complement(s).encode()


def test_every_pair_of_starts_on_every_kind_of_tile():
    seen = {k: set() for k in rcc.KINDS}
    for b in rcc.batches():
        for t in rcc.tiles(b.reads):
            assert t.n >= 1 and t.d0 - t.i0 - sum(len(r) for r in b.reads) == rcc.offsets(b.reads)[t.read]
            if rcc.kind(t):
                seen[rcc.kind(t)].add((t.s0 & 3, t.d0 & 3))
    every = {(s, d) for s in range(4) for d in range(4)}
    for k in rcc.KINDS:
        assert seen[k] == every, (k, sorted(every - seen[k]))
    assert {t.n for b in rcc.batches() for t in rcc.tiles(b.reads) if rcc.kind(t) == "shorter than 4"} == {1, 2, 3}
    assert {t.n % 4 for b in rcc.batches() for t in rcc.tiles(b.reads) if rcc.kind(t) == "not a multiple of 4"} == {1, 2, 3}


def test_lengths_totals_and_empty_reads():
    bs = {b.name: b.reads for b in rcc.batches()}
    assert bs["no-reads"] == () and bs["all-empty"] == (b"",) * 3
    for m in range(4):
        reads = bs["total-%d-mod-4" % m]
        assert sum(len(r) for r in reads) % 4 == m
        assert set(map(len, reads)) == set(rcc.LENGTHS)
        assert reads[0] == b"" and reads[-1] == b"" and b"" in reads[1:-1]
        assert all(reads.count(r) == 1 for r in reads if len(r) > 8)
    assert rcc.LENGTHS == (0, 1, 2, 3, 4, 5, 7, 8, 1020, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 1028, 2047, 2048, 2049, 3071, 3072, 3073, 5000)
    assert rcc.batches() is rcc.batches() and rcc.batches.__wrapped__()[0].reads == rcc.batches()[0].reads


def test_contents():
    for b in rcc.batches()[:4]:
        assert any(set(r) == set(range(256)) for r in b.reads), "a read of all 256 byte values"
        assert any(len(r) >= 1020 and set(r) <= set(b"ACGT") for r in b.reads), "random ACGT"
        mixed = [r for r in b.reads if len(r) >= 1020 and set(r) <= set(b"ACGTacgtUuNn") and not set(r) <= set(b"ACGT")]
        assert mixed and all(set(b"acgtUuN") <= set(r) for r in mixed), "lower case, U, u and N"


def test_tile_of():
    reads = rcc.batches()[1].reads
    r = next(i for i, x in enumerate(reads) if len(x) == 5000)
    off, total = rcc.offsets(reads), sum(len(x) for x in reads)
    assert [rcc.tile_of(reads, r, b).i0 for b in (0, 1023, 1024, 4999)] == [0, 0, 1024, 4096]
    t = rcc.tile_of(reads, r, 4999)
    assert (t.s0, t.d0, t.n) == (off[r], total + off[r] + 4096, 904)
