"""Seeded alignment cases for k_dl_events (csrc/vga_deletion.hip), which reads a traceback's operations forward in blocks of 64 and
emits a deletion run at the lane that closes it.  Built on op_cases.Edit: on the one-node graph DRB5 the column of graph base p is
p plus the read bases inserted before it, so an Edit script puts the first D of a run, and with its length the closing operation,
on the lane it names.  `conditions` derives from the oracle's alignments GAF alone which of the conditions the sets are there for
are present; tests/test_deletion_cpu.py asserts them.

The sets:
  drb5-del-lanes    runs whose first D is on lane 0 and on lane 63, runs whose closing operation is on lane 0 and on lane 63
  drb5-del-blocks   runs of exactly 63, 64, 65, 128 and 129 D, each from lane 0, from lane 1 and from lane 63: a run inside one
                    block, over two and over three
  drb5-del-pairs    two runs separated by a single match that sits on lane 63, and on lane 0
  drb1-del-ins      op_cases' replaced-window reads: a run directly before an insertion
  drb1-del-nodes    70 deleted path bases on DRB1 (op_cases.sweep_reads): runs that cross several node boundaries
  synth-del-nodes   reads of the synthetic pangenome (32-bp nodes) with 10 and with 70 path bases cut out: runs that cross one node
                    boundary and several
planted_reads is the sample of the README's example: a deletion of twelve bases planted in the middle of a DRB1 node.
Every read of a DRB5 set begins and ends with a deletion (the alignment is global over the node): a run as the first graph-consuming
token and one as the last, the end runs.

Not produced by the aligner, and so not here: a run directly BEHIND an insertion.  Wherever an insertion and a deletion meet the
two can change places at no cost, and on these reads the oracle writes the deletion first (op_cases.replaced_window_reads, and
tests/test_insertion_gpu.py found the same from the other side).  conditions() still reports it, and test_deletion_cpu.py prints
whether any set holds one."""
import re

import op_cases as M

LANE_RUNS = ((0, 3), (63, 2), (61, 3), (60, 3), (0, 64), (63, 1))   # (lane of the first D, length): closing on 3, 1, 0, 63, 0, 0
BLOCK_LENGTHS = (63, 64, 65, 128, 129)
BLOCK_LANES = (0, 1, 63)


def lane_case():
    h = M._first_path("drb5")
    reads = []
    for i, (lane, n) in enumerate(LANE_RUNS):
        e = M.Edit(h, 900 + 700 * i)
        e.delete(lane, n, gap=150)
        reads.append(e.read(gap=200))
    return M.Case("drb5-del-lanes", "drb5", M.K, reads, False)


def block_case():
    h = M._first_path("drb5")
    reads = []
    for i, n in enumerate(BLOCK_LENGTHS):
        for j, lane in enumerate(BLOCK_LANES):
            e = M.Edit(h, 500 + 800 * i + 2000 * j)
            e.delete(lane, n, gap=200)
            reads.append(e.read(gap=300))
    return M.Case("drb5-del-blocks", "drb5", M.K, reads, False)


def pair_case():
    """D3 =1 D3 with the single match on lane 63 and on lane 0: two gaps of three cost less than one of seven and a mismatch"""
    h = M._first_path("drb5")
    reads = []
    for i, lane in enumerate((63, 0)):
        for k in range(4):   # a few places each: a place where the pair can be written another way gives another record
            e = M.Edit(h, 1500 + 2500 * i + 600 * k)
            e.delete(lane - 3, 3, gap=200)
            p = e.p   # the single match, on `lane`
            ok = lambda q: h[q + 1] != h[q + 4] and h[q] != h[q + 3] and h[q] != h[q - 3] and h[q] != h[q + 4]
            if not ok(p):
                continue
            e.copy_to(p + 1)
            e.p = p + 4
            reads.append(e.read(gap=300))
    return M.Case("drb5-del-pairs", "drb5", M.K, reads, False)


def del_ins_case():
    hap = M._first_path("drb1")
    reads = M.replaced_window_reads(hap)
    n0 = M.REPLACED_WINDOWS[0][1]
    return M.Case("drb1-del-ins", "drb1", M.K, [reads[0], reads[5], reads[n0], reads[n0 + 3]], False)


def node_case():
    return M.Case("drb1-del-nodes", "drb1", M.K, M.sweep_reads(M._first_path("drb1"), start=2600, n=6), False)


def synth_case(tmp_dir):
    gfa = M.gfa_path(M.Case("", "synth", M.K, (), False), tmp_dir)
    exact = [r.seq for r in M._readsim().simulate_reads(gfa, 8, 700, 0.0, 0.0, 0.0, seed=15)]
    reads = [s[:300] + s[300 + (10 if i % 2 else 70):] for i, s in enumerate(exact)]
    return M.Case("synth-del-nodes", "synth", M.K, reads, False)


def all_cases(tmp_dir):
    return [lane_case(), block_case(), pair_case(), del_ins_case(), node_case(), synth_case(tmp_dir)]


PLANTED = 12


def planted_reads(node_seq_idx, n_reads=12, length=1000):
    """A sample from path 3 of DRB1 whose sequence lacks PLANTED bases centred on the middle of a node (the set-up of
    tests/test_insertion_cpu.py): n_reads reads of `length` bases with 1 % of each error, tiled so that the site moves through the
    read ("hom"); and the same with as many reads of the unchanged path interleaved ("het").
    -> (node id, graph position of the first deleted base, {sample: [(name, read)]})"""
    import numpy as np

    rs = M._readsim()
    idx = [int(x) for x in node_seq_idx]
    segs, paths = rs.parse_gfa_paths(M.GRAPHS["drb1"])
    name, steps = paths[3]
    assert not any(rev for _, rev in steps)
    off = 0
    for nid, _ in steps:
        if off >= 2000 and len(segs[nid]) >= 50:
            break
        off += len(segs[nid])
    middle = len(segs[nid]) // 2 - PLANTED // 2
    site_path, site_graph = off + middle, idx[nid - 1] + middle
    seq = rs.path_sequence(segs, steps)
    assert idx[nid - 1] < site_graph and site_graph + PLANTED < idx[nid]
    mut = seq[:site_path] + seq[site_path + PLANTED:]
    out = {}
    for sample, sources in (("hom", (mut,)), ("het", (mut, seq))):
        rng = np.random.Generator(np.random.PCG64(11))
        reads = []
        for r in range(n_reads):
            o = site_path - length + (r + 1) * length // (n_reads + 1)
            for s in sources:
                tpl = np.frombuffer(s[o:o + length].encode(), dtype=np.uint8)
                reads.append(("%s%d_%d" % (sample, r, len(reads)), rs._mutate(tpl, rng, 0.01, 0.01, 0.01).decode()))
        out[sample] = reads
    return nid, site_graph, out


def conditions(gaf_text, node_len):
    """what an alignments GAF holds, from its text alone -> a dict of sets and counts"""
    out = {"first_lane": set(), "closing_lane": set(), "lengths": set(), "blocks": set(), "pair_lane": set(), "before_ins": 0, "behind_ins": 0,
           "leading": 0, "trailing": 0, "crossings": set()}
    for rec, line in zip(M.properties(gaf_text, node_len), gaf_text.splitlines()):
        if rec is None:
            continue
        cs = re.search(r"cs:Z:([^,\s]*)", line).group(1)
        out["before_ins"] += len(re.findall(r"-[a-z]+\+", cs))
        out["behind_ins"] += len(re.findall(r"\+[a-z]+-", cs))
        rr = M.runs(rec)
        consuming = [k for k, (kind, _, _) in enumerate(rr) if kind != "I"]
        entry_at = sorted(e[0] for e in rec.entries[1:])
        for k, (kind, f, n) in enumerate(rr):
            if kind != "D":
                continue
            if k == consuming[0]:
                out["leading"] += 1
                continue
            if k == consuming[-1]:
                out["trailing"] += 1
                continue
            out["first_lane"].add(f % 64)
            out["closing_lane"].add((f + n) % 64)
            out["lengths"].add(n)
            out["blocks"].add((n, (f + n) // 64 - f // 64))
            out["crossings"].add(sum(f < e < f + n for e in entry_at))
            # D run, one E, D run: the lane of the single match
            if k + 2 < len(rr) and rr[k + 1] == ("E", f + n, 1) and rr[k + 2][0] == "D":
                out["pair_lane"].add((f + n) % 64)
    return out
