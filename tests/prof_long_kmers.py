"""diagnostic: what the hashed probe table (k = 16..32) costs and what a longer seed buys.  One context,
one JSON object on stdout (profiles/long_kmers.json).

  hash_cost     k = 15 on config 3 (DRB1-3123) and config 5 (1 Mbp synthetic pangenome): the same index uploaded twice, once
                with the direct-address table and once with VGA_PROBE_TABLE=hash, the same reads, K1's count + emit time per
                step from the library's own timers (kmer_probe_count / kmer_probe_emit), the order of the two swapped
                between repeats.
  longer_seed   config 5 at k = 11, 15, 19 and config 3 at k = 11, 19: aligned reads/s over the timed steps (map + align, the
                step bench.py times: warm-up steps, synchronise, wall clock over the steps), anchors per read, K1 / K2 / K3 ms per
                step, and the share of reads whose alignment path agrees with the simulated truth (node-range Jaccard >= 0.9
                against readsim.truth_gaf, gafcompare's metric).
  probe_memory  device bytes of the probe tables and of the position arrays per index, from the allocation sizes the upload
                reports under VGA_TRACE=1 (each upload runs in a child process whose stderr is read), against 4^k * 4, one
                direct-address table (k <= 13 has two of them, the hashed table serves both views; its position bytes hold
                both position arrays).

    python tests/prof_long_kmers.py [--reads3 10000] [--reads5 10000] [--steps 5] [--warmup 1] [--repeats 4]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

p = ge.load_package()
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
K1 = ("kmer_probe_count", "kmer_probe_emit")


def kernel_ms(st, names):
    return sum(k["ms"] for k in st["kernels"] if k["name"] in names)


def upload(hidx, ctx, hashed):
    if hashed:
        os.environ["VGA_PROBE_TABLE"] = "hash"  # read at upload time
    try:
        hidx.upload(ctx)
    finally:
        os.environ.pop("VGA_PROBE_TABLE", None)


def hash_cost(gfa, seqs, steps, repeats):
    hidx = p.HostIndex.build_from_gfa(gfa, 15)
    ctxs = {"direct": p.Context(0), "hash": p.Context(0)}
    upload(hidx, ctxs["direct"], False)
    upload(hidx, ctxs["hash"], True)
    batches = {n: c.batch(seqs) for n, c in ctxs.items()}
    mp = p.default_map_params()
    mp.emit_dp = 0
    per = {"direct": [], "hash": []}
    n_anchors = {}
    for n in per:  # warm-up: workspaces grow
        n_anchors[n] = batches[n].map_raw(mp)["n_anchors"]
    for rep in range(repeats):
        for n in (("direct", "hash") if rep % 2 == 0 else ("hash", "direct")):
            ms = [kernel_ms(batches[n].map_raw(mp), K1) for _ in range(steps)]
            per[n].append(round(float(np.mean(ms)), 4))
    for n in per:
        batches[n].close()
        ctxs[n].close()
    assert n_anchors["direct"] == n_anchors["hash"]
    return {"k": 15, "reads": len(seqs), "anchors": n_anchors["direct"], "steps_per_repeat": steps,
            "k1_ms_per_step_direct": per["direct"], "k1_ms_per_step_hash": per["hash"],
            "ratio_of_means": round(float(np.mean(per["hash"]) / np.mean(per["direct"])), 3)}


def true_path_share(gfa, reads, al):
    gc = p.gafcompare
    truth = p.readsim.truth_gaf(gfa, reads).splitlines()
    ok = 0
    for r, t in enumerate(truth):
        if not al.aligned[r]:
            continue
        hs = al.path_handles[int(al.path_off[r]):int(al.path_off[r + 1])].tolist()
        ok += gc.jaccard([(h >> 1) * (-1 if h & 1 else 1) for h in hs], gc.signed_path(t.split("\t")[5])) >= 0.9
    return ok / len(reads)


def longer_seed(gfa, reads, k, steps, warmup):
    t0 = time.time()
    hidx = p.HostIndex.build_from_gfa(gfa, k)
    t_index = time.time() - t0
    ctx = p.Context(0)
    hidx.upload(ctx)
    seqs = [r.seq for r in reads]
    b = ctx.batch(seqs)
    mo = b.map()
    al = b.align(mo)
    out = {"k": k, "reads": len(reads), "host_index_build_s": round(t_index, 2), "anchors_per_read": round(mo.n_anchors / len(reads), 1),
           "aligned": int(np.asarray(al.aligned).sum()), "true_path_share": round(true_path_share(gfa, reads, al), 4)}
    del mo, al
    for _ in range(warmup):
        b.map_align_raw()
    ctx.synchronize()
    sums = {"k1": 0.0, "k2_anchor_sort": 0.0, "k3_chain": 0.0, "map": 0.0}
    aligned = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        st = b.map_align_raw()
        aligned += st["aligned"]
        sums["k1"] += kernel_ms(st, K1)
        sums["k2_anchor_sort"] += st["ms_sort"]
        sums["k3_chain"] += st["ms_chain"]
        sums["map"] += st["ms_map"]
    ctx.synchronize()
    dt = time.perf_counter() - t0
    out["aligned_reads_per_s"] = round(aligned / dt, 1)
    out["ms_per_step"] = round(dt / steps * 1e3, 1)
    out["ms_per_step_kernels"] = {n: round(v / steps, 3) for n, v in sums.items()}
    b.close()
    ctx.close()
    return out


def probe_memory(gfa, k, hashed):
    """the upload's own report of its allocations, from a child process run with VGA_TRACE=1"""
    code = ("import sys; sys.path.insert(0, %r); import __graft_entry__ as ge; p = ge.load_package(); "
            "h = p.HostIndex.build_from_gfa(%r, %d); c = p.Context(0); h.upload(c); c.close()" % (ROOT, gfa, k))
    env = dict(os.environ, VGA_TRACE="1")
    if hashed:
        env["VGA_PROBE_TABLE"] = "hash"
    err = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900).stderr
    m = re.search(r"index_upload: k (\d+) (\w+) probe table (\d+) bytes, positions (\d+) bytes, (\d+) k-mers", err)
    if not m:
        return {"k": k, "error": err[-300:]}
    return {"k": k, "kind": m.group(2), "probe_table_bytes": int(m.group(3)), "position_bytes": int(m.group(4)), "kmers": int(m.group(5)),
            "one_direct_table_bytes": 4 ** k * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads3", type=int, default=10000)
    ap.add_argument("--reads5", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--parts", default="hash_cost,longer_seed,probe_memory")
    a = ap.parse_args()
    os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
    cfg5 = os.path.join(tempfile.mkdtemp(prefix="vga_long_kmers_"), "config5.gfa")
    p.readsim.synth_pangenome(cfg5)
    reads3 = p.readsim.config3_reads(DRB1, a.reads3)
    reads5 = p.readsim.config3_reads(cfg5, a.reads5)
    res = {"command": "python tests/prof_long_kmers.py " + " ".join(sys.argv[1:]),
           "workloads": {"config3": "DRB1-3123, %d x 10 kbp reads, 3/3/4 %% sub/ins/del, seed 77" % a.reads3,
                         "config5": "1 Mbp synthetic pangenome (readsim.synth_pangenome), %d x 10 kbp reads, same read model" % a.reads5},
           "steps": a.steps, "warmup": a.warmup}
    parts = a.parts.split(",")
    if "hash_cost" in parts:
        res["hash_cost"] = {"config3": hash_cost(DRB1, [r.seq for r in reads3], a.steps, a.repeats),
                            "config5": hash_cost(cfg5, [r.seq for r in reads5], a.steps, a.repeats)}
        print(json.dumps(res["hash_cost"]), file=sys.stderr, flush=True)
    if "longer_seed" in parts:
        res["longer_seed"] = {"config5": [], "config3": []}
        for k in (11, 15, 19):
            res["longer_seed"]["config5"].append(longer_seed(cfg5, reads5, k, a.steps, a.warmup))
            print(json.dumps(res["longer_seed"]["config5"][-1]), file=sys.stderr, flush=True)
        for k in (11, 19):
            res["longer_seed"]["config3"].append(longer_seed(DRB1, reads3, k, a.steps, a.warmup))
            print(json.dumps(res["longer_seed"]["config3"][-1]), file=sys.stderr, flush=True)
    if "probe_memory" in parts:
        res["probe_memory"] = {"config3": [probe_memory(DRB1, k, False) for k in (11, 15, 16, 19, 24, 32)] + [probe_memory(DRB1, 15, True)],
                               "config5": [probe_memory(cfg5, k, False) for k in (11, 19, 32)]}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
