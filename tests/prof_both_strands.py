"""diagnostic: vga_map_params.strands = VGA_STRANDS_BOTH on config 3 (10 000 x 10 kbp ONT-like reads vs DRB1-3123, seed 77, one
context).  Three runs:
  (i)   forward mode on a read set with reverse_fraction = 0.5;
  (ii)  both mode on the same set;
  (iii) forward mode on the all-forward set (bench.py's workload).
Per run: aligned reads, reads aligned to their true path (node-path Jaccard >= 0.9 against readsim.truth_gaf, gafcompare's
metric) and the mean Jaccard, aligned reads/s over the timed steps (map + align, as bench.py times a step), map ms, and the new
kernels' ms (revcomp_reads, strand_pick, strand_gather) from vga_last_kernel_times -- per timed step, and in the first map call
of the batch, the one that builds its reverse complement; for (ii) the share of picked strands that equal the simulated ones.
One JSON object on stdout.

    python tests/prof_both_strands.py [--reads 10000] [--steps 3] [--warmup 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

p = ge.load_package()
GFA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "DRB1-3123.gfa")
NEW_KERNELS = ("revcomp_reads", "strand_pick", "strand_gather")


def jaccards(reads, al, truth):
    """per read, gafcompare's node-range Jaccard index of the alignment path against the truth (0 when not aligned)"""
    gc = p.gafcompare
    out = []
    for r, t in zip(range(len(reads)), truth.splitlines()):
        hs = al.path_handles[int(al.path_off[r]):int(al.path_off[r + 1])].tolist() if al.aligned[r] else []
        out.append(gc.jaccard([(h >> 1) * (-1 if h & 1 else 1) for h in hs], gc.signed_path(t.split("\t")[5])))
    return np.array(out)


def run(ctx, reads, strands, steps, warmup):
    seqs = [r.seq for r in reads]
    b = ctx.batch(seqs)
    mp = p.default_map_params()
    mp.emit_dp = 0
    mp.strands = strands
    # one untimed step with the results kept: what was aligned where
    mo = b.map(mp)
    first = {k["name"]: round(k["ms"], 4) for k in ctx.kernel_times() if k["name"] in NEW_KERNELS}
    al = b.align(mo)
    jac = jaccards(reads, al, p.readsim.truth_gaf(GFA, reads))
    out = {"aligned": int(al.aligned.sum()), "aligned_to_true_path": int((jac >= 0.9).sum()), "mean_jaccard": round(float(jac.mean()), 4),
           "new_kernels_ms_first_map_call": first}
    if mo.strand is not None:
        want = np.array([1 if r.strand == "-" else 0 for r in reads], dtype=np.uint8)
        out["reverse_picked"] = int(mo.strand.sum())
        out["strand_recall"] = float((mo.strand == want).mean())
    del mo, al
    for _ in range(warmup):
        b.map_align_raw(map_params=mp)
    ctx.synchronize()
    ms_map, kern, aligned = [], {k: 0.0 for k in NEW_KERNELS}, 0
    t0 = time.perf_counter()
    for _ in range(steps):
        st = b.map_align_raw(map_params=mp)
        ms_map.append(st["ms_map"])
        aligned += st["aligned"]
        for k in st["kernels"]:
            if k["name"] in kern:
                kern[k["name"]] += k["ms"]
    ctx.synchronize()
    dt = time.perf_counter() - t0
    out.update({"aligned_reads_per_s": round(aligned / dt, 1), "map_ms": round(float(np.mean(ms_map)), 2),
                "new_kernels_ms_per_step": {k: round(v / steps, 4) for k, v in kern.items()}})
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    sim = p.readsim.simulate_reads
    mixed = sim(GFA, a.reads, 10000, 0.03, 0.03, 0.04, seed=77, reverse_fraction=0.5)
    fwd = p.readsim.config3_reads(GFA, a.reads)
    hidx = p.HostIndex.build_from_gfa(GFA, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    F, B = p.binding.VGA_STRANDS_FORWARD, p.binding.VGA_STRANDS_BOTH
    res = {"workload": "config3: %d x 10 kbp, 3/3/4 %% sub/ins/del, seed 77, DRB1-3123, k = 11" % a.reads, "steps": a.steps,
           "i_forward_on_mixed": run(ctx, mixed, F, a.steps, a.warmup),
           "ii_both_on_mixed": run(ctx, mixed, B, a.steps, a.warmup),
           "iii_forward_on_forward": run(ctx, fwd, F, a.steps, a.warmup)}
    res["reverse_reads_in_mixed"] = sum(r.strand == "-" for r in mixed)
    ctx.close()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
