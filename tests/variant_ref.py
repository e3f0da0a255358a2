"""Plain reference for the variant call: what vga_variant_call / vga_variant_call_table return, from a pileup table and the
letters of its bases (call_table), or from the text of an alignments GAF through pileup_ref.walk (call_gaf), and from nothing
else.  Written from the definition in include/vga_hip.h with Python integers; it shares no code with the product (test
infrastructure).

Per base, with its row A C G T N del ins and r = the column of its own letter:
    depth = A + C + G + T + N + del; the alleles are A < C < G < T < D with n_D = del; N counts towards depth only
    tested: r < 4 and depth >= min_depth
    cost(x, y) over the 15 pairs x <= y: a homozygous pair pays 0 for an observation of x and E for any other, a heterozygous one
        256 for x or y and E for any other.  Order: (r, r), the four pairs that hold r by their other allele, the other ten by
        (x, y); the first minimum is the genotype, qual = the smallest of the other fourteen minus it, saturated at 2^32 - 1
    insertion: k = min(ins, depth); none costs ins E, het 256 depth, hom (depth - k) E; first minimum in that order, ins_qual =
        the second smallest minus it
    reported: tested, and (genotype != (r, r) and qual >= min_qual) or (state != none and ins_qual >= min_qual)"""
import functools

import numpy as np

import pileup_ref

ERROR, MIN_DEPTH, MIN_QUAL = 1280, 4, 512
ALLELES = "ACGT-"
INS_STATES = (".", "het", "hom")
HEADER = "node\toffset\tref\tgt\tqual\tins\tins_qual\tdepth\tA\tC\tG\tT\tN\tdel\tins_count"
QUAL_MAX = 2**32 - 1


def pair_order(r):
    """the 15 pairs in the order of the definition for a base whose own allele is r"""
    order = [(r, r)] + [(min(r, o), max(r, o)) for o in range(5) if o != r]
    return order + [(x, y) for x in range(5) for y in range(x, 5) if x != r and y != r]


def weight(a, x, y, error):
    """the cost of one observation of allele a under the genotype (x, y)"""
    if x == y:
        return 0 if a == x else error
    return 256 if a in (x, y) else error


@functools.lru_cache(maxsize=None)
def pair_weights(r, error):
    """[((x, y), (w_A, w_C, w_G, w_T, w_D))] in the order of the definition"""
    return [((x, y), tuple(weight(a, x, y, error) for a in range(5))) for x, y in pair_order(r)]


def site(row, letter, error=ERROR, min_depth=MIN_DEPTH, min_qual=MIN_QUAL):
    """one base -> dict(tested, reported, x, y, ins, qual, ins_qual, depth)"""
    row = [int(v) for v in row]
    n = row[0:4] + [row[5]]
    ins = row[6]
    depth = sum(row[0:6])
    r = pileup_ref.column(letter if isinstance(letter, str) else chr(letter))
    out = {"depth": depth, "tested": r < 4 and depth >= min_depth, "reported": False}
    if r >= 4:
        return out
    pairs = pair_weights(r, error)
    costs = [n[0] * w[0] + n[1] * w[1] + n[2] * w[2] + n[3] * w[3] + n[4] * w[4] for _, w in pairs]
    best = costs.index(min(costs))  # the first minimum
    out["x"], out["y"] = pairs[best][0]
    out["qual"] = min(min(costs[:best] + costs[best + 1:]) - costs[best], QUAL_MAX)
    k = min(ins, depth)
    ic = [ins * error, 256 * depth, (depth - k) * error]
    state = ic.index(min(ic))
    out["ins"] = state
    out["ins_qual"] = sorted(ic)[1] - ic[state]
    out["reported"] = out["tested"] and (((out["x"], out["y"]) != (r, r) and out["qual"] >= min_qual) or
                                         (state != 0 and out["ins_qual"] >= min_qual))
    return out


def call_table(counts, letters, error=ERROR, min_depth=MIN_DEPTH, min_qual=MIN_QUAL):
    """-> the dict Context.variant_call_table returns: arrays over the reported bases in base order, n_tested, n_calls"""
    if isinstance(letters, (bytes, bytearray)):
        letters = letters.decode()
    rows = [[int(v) for v in row] for row in np.asarray(counts, dtype=object).reshape(-1, 7).tolist()]
    assert len(rows) == len(letters)
    keep, n_tested = [], 0
    for i, (row, letter) in enumerate(zip(rows, letters)):
        s = site(row, letter, error, min_depth, min_qual)
        n_tested += s["tested"]
        if s["reported"]:
            keep.append((i, s, row))
    return {"pos": np.array([i for i, _, _ in keep], dtype=np.uint32),
            "x": np.array([s["x"] for _, s, _ in keep], dtype=np.uint8), "y": np.array([s["y"] for _, s, _ in keep], dtype=np.uint8),
            "ins": np.array([s["ins"] for _, s, _ in keep], dtype=np.uint8),
            "qual": np.array([s["qual"] for _, s, _ in keep], dtype=np.uint32),
            "ins_qual": np.array([s["ins_qual"] for _, s, _ in keep], dtype=np.uint64),
            "depth": np.array([s["depth"] for _, s, _ in keep], dtype=np.uint64),
            "counts": np.array([row for _, _, row in keep], dtype=np.uint64).reshape(-1, 7),
            "n_tested": int(n_tested), "n_calls": len(keep)}


def call_gaf(gaf_text, node_seq_idx, seq_fwd, error=ERROR, min_depth=MIN_DEPTH, min_qual=MIN_QUAL):
    """the same from the alignments GAF alone"""
    counts, _, _ = pileup_ref.walk(gaf_text, node_seq_idx, seq_fwd)
    return call_table(counts, seq_fwd, error, min_depth, min_qual)


def same(a, b):
    """two result dicts agree exactly; returns the name of the first field that differs, or None"""
    for k in ("n_tested", "n_calls"):
        if int(a[k]) != int(b[k]):
            return k
    for k in ("pos", "x", "y", "ins", "qual", "ins_qual", "depth", "counts"):
        if np.asarray(a[k]).shape != np.asarray(b[k]).shape or not np.array_equal(np.asarray(a[k]).astype(object), np.asarray(b[k]).astype(object)):
            return k
    return None


def tsv(calls, node_seq_idx, seq_fwd):
    """the text of <out>-variants.tsv for a result dict"""
    idx = np.asarray([int(x) for x in node_seq_idx], dtype=np.int64)
    seq = seq_fwd.decode() if isinstance(seq_fwd, (bytes, bytearray)) else str(seq_fwd)
    lines = [HEADER]
    for j in range(int(len(calls["pos"]))):
        p = int(calls["pos"][j])
        node = int(np.searchsorted(idx, p, side="right"))  # 1-based id of the node that holds p
        f = [node, p - int(idx[node - 1]), seq[p], ALLELES[int(calls["x"][j])] + "/" + ALLELES[int(calls["y"][j])], int(calls["qual"][j]),
             INS_STATES[int(calls["ins"][j])], int(calls["ins_qual"][j]), int(calls["depth"][j])] + [int(v) for v in calls["counts"][j]]
        lines.append("\t".join(str(v) for v in f))
    return "\n".join(lines) + "\n"
