"""Seeded read batches for k_revcomp_reads (csrc/vga_strand.hip) and the host route beside it, read back through the seam
vga_batch_strands, and a plain reference of the reverse complement.  The kernel stages the mirrored window of a 1 024-byte tile
with 32-bit loads from the word that holds its first byte and writes full words, with byte stores at the head and tail of the
tile; reads start at any byte offset.  So what matters is where a tile's source and destination start inside a word, and how
long the last tile is -- and bytes that simulated reads never hold.  Plain Python: no GPU, no oracle, nothing from the product."""
import functools
import random
from collections import namedtuple

TILE = 1024  # output bytes per tile (VGA_RC_TILE)

# the reference's switch_base (src/dna.rs:20-33), written out: A<->T, C<->G, a<->t, c<->g, U->A, u->a, every other byte N
TABLE = [ord("N")] * 256
for _a, _b in ((b"A", b"T"), (b"T", b"A"), (b"C", b"G"), (b"G", b"C"), (b"a", b"t"), (b"t", b"a"), (b"c", b"g"), (b"g", b"c"), (b"U", b"A"), (b"u", b"a")):
    TABLE[_a[0]] = _b[0]
TABLE = tuple(TABLE)

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8) + tuple(range(1020, 1029)) + (2047, 2048, 2049, 3071, 3072, 3073, 5000)
COPIES = 3  # of every length in a batch, so that each kind of tile meets each start inside a word

Batch = namedtuple("Batch", "name reads")
Tile = namedtuple("Tile", "read i0 s0 d0 n")


def reverse_complement(read):
    return bytes(TABLE[c] for c in reversed(read))


def offsets(reads):
    off = [0]
    for r in reads:
        off.append(off[-1] + len(r))
    return off


def tiles(reads):
    """every tile of every read as the kernel's comment defines it: forward bytes [s0, s0 + n) of the batch become bytes
    [d0, d0 + n) of the allocation, mirrored; d0 counts from the start of the forward half, the reverse half starts at total"""
    off = offsets(reads)
    total = off[-1]
    out = []
    for r, read in enumerate(reads):
        L = len(read)
        for i0 in range(0, L, TILE):
            n = min(TILE, L - i0)
            out.append(Tile(r, i0, off[r] + L - i0 - n, total + off[r] + i0, n))
    return out


def tile_of(reads, read, byte):
    """the tile that writes byte `byte` of the reverse complement of read `read`"""
    i0 = byte // TILE * TILE
    return next(t for t in tiles(reads) if t.read == read and t.i0 == i0)


KINDS = ("full", "shorter than 4", "not a multiple of 4")


def kind(t):
    """which of the three kinds of tile the coverage is asked for; None for the rest (a last tile of 4 k bytes, k < 256)"""
    if t.n == TILE:
        return "full"
    if t.n < 4:
        return "shorter than 4"
    return "not a multiple of 4" if t.n % 4 else None


def _content(rng, n, which):
    if which == "bytes":  # every byte value, as often as the length allows, in a seeded order
        vals = [i % 256 for i in range(n)]
        rng.shuffle(vals)
        return bytes(vals)
    alphabet = b"ACGT" if which == "acgt" else b"ACGTacgtUuNn"
    return bytes(rng.choice(alphabet) for _ in range(n))


def _build(total_mod4, seed):
    rng = random.Random(seed)
    lengths = [n for n in LENGTHS if n] * COPIES
    rng.shuffle(lengths)
    reads = []
    for i, n in enumerate(lengths):
        which = "bytes" if (n >= 1024 and i % 3 == 0) else ("mixed" if i % 3 == 1 else "acgt")
        reads.append(_content(rng, n, which))
    reads.insert(len(reads) // 2, b"")
    pad = (total_mod4 - sum(len(r) for r in reads)) % 4
    if pad:
        reads.append(_content(rng, pad, "mixed"))
    return [b""] + reads + [b""]


def _kinds_at_every_source_start(reads):
    return {(kind(t), t.s0 & 3) for t in tiles(reads)} >= {(k, s) for k in KINDS for s in range(4)}


@functools.lru_cache(maxsize=None)
def batches(seed=6100):
    """four batches whose totals are 0, 1, 2 and 3 mod 4 -- the last tile of a read starts at the read's own offset, so its
    destination is `total` bytes further and only the four totals together give every pair of starts -- then a batch of no reads
    and one whose reads are all empty.  Each of the four: every length of LENGTHS three times in a seeded order, an empty read
    first, in the middle and last; the first seed from `seed` on at which every kind of tile meets every source start."""
    out = []
    for m in range(4):
        s = seed + 100 * m
        while not _kinds_at_every_source_start(_build(m, s)):
            s += 1
        out.append(Batch("total-%d-mod-4" % m, tuple(_build(m, s))))
    out.append(Batch("no-reads", ()))
    out.append(Batch("all-empty", (b"", b"", b"")))
    return tuple(out)
