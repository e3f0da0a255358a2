"""diagnostic: what path support costs.  One JSON object on stdout (profiles/path_support.json).
Every measurement runs in a child process of its own, and the processes of a pair alternate, so that both sides of a comparison
see the same box in the same minutes.  `--parent-lib` names a libvga_hip.so built from the parent commit (the binding's VGA_LIB).

  bench_ab   off costs nothing: `python bench.py` (config 3) with this tree's library and with the parent's, alternating,
             `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  step       the on-cost: config 3 (12 paths) and config 5 (16 paths) steps (10 000 x 10 kbp reads, seed 77: map + align, the step
             bench.py times) with path support off and on, same library, alternating; aligned reads/s, the time of
             vga_path_support_begin with k_ps_build in it, and from vga_last_kernel_times the busy time per step of k_cov_runs
             (the lists, made for path support as for coverage), k_ps_score, poa_text and poa_band_dp.
  many       how the cost grows with the words per bitset: one call of the seam vga_path_support_lists on the config 5 graph, the
             same `--lists` edge-following lists of `--list-nodes` nodes against 16, 64, 256, 1024 and 4096 synthetic paths.

    python tests/prof_path_support.py --parent-lib PATH [--parts bench_ab,step,many] [--repeats 4] [--reads 10000] [--steps 3]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
BUSY = ("k_cov_runs", "k_ps_score", "k_cov_add", "poa_text", "poa_band_dp")


def child_step(gfa, n_reads, steps, warmup, on):
    """one process: reads/s of the timed steps and the kernels' busy time per step"""
    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(gfa, n_reads)])
    out = {}
    if on:
        g = p.hostlib.gfa_paths(gfa)
        t0 = time.perf_counter()
        missing = ctx.path_support_begin(g["step_off"], g["steps"])
        out["begin"] = {"paths": len(g["names"]), "steps": int(g["step_off"][-1]), "pairs_without_edge": missing,
                        "begin_ms": round((time.perf_counter() - t0) * 1e3, 3),
                        "k_ps_build_ms": round(sum(k["ms"] for k in ctx.kernel_times() if k["name"] == "k_ps_build"), 4)}
    for _ in range(warmup):
        b.map_align_raw()
    ctx.synchronize()
    if on:
        ctx.path_support_reset()
    busy = {n: 0.0 for n in BUSY}
    aligned = 0
    t0 = time.perf_counter()
    for _ in range(steps):
        st = b.map_align_raw()
        aligned += st["aligned"]
        for k in st["kernels"]:
            if k["name"] in busy:
                busy[k["name"]] += k["busy_ms"]
    ctx.synchronize()
    dt = time.perf_counter() - t0
    out.update({"aligned_reads_per_s": round(aligned / dt, 1), "ms_per_step": round(dt / steps * 1e3, 1),
                "busy_ms_per_step": {n: round(v / steps, 3) for n, v in busy.items()}})
    if on:
        acc = ctx.path_support()
        out["scored"] = {"alignments": acc["n_alignments"], "unplaced": acc["n_unplaced"], "sum_bases": int(acc["sum_bases"].sum()),
                         "sum_edges": int(acc["sum_edges"].sum()), "top": int(acc["top"].sum()), "top_alone": int(acc["top_alone"].sum())}
    print(json.dumps(out), flush=True)


def child_many(gfa, n_lists, list_nodes):
    """one process: the seam on the graph of `gfa` against more and more synthetic paths (random edge-following walks)"""
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    a = hidx.arrays()
    ctx = p.Context(0)
    hidx.upload(ctx)
    idx, eidx, eto, edg = a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"]
    n_nodes = len(idx) - 1
    rng = np.random.default_rng(7)

    def follow(start, n):
        l = [start]
        while len(l) < n:
            out = edg[int(eidx[l[-1] - 1] + eto[l[-1] - 1]):int(eidx[l[-1]])]
            out = out[(out & 1) == 0]
            if len(out) == 0:
                break
            l.append(int(out[int(rng.integers(0, len(out)))]) >> 1)
        return l

    walks = [np.asarray(follow(1, n_nodes), dtype=np.uint64) for _ in range(16)]  # haplotypes: walks through the whole graph
    lists, bases = [], []
    for i in range(n_lists):  # windows of the haplotypes, fully covered
        w = walks[i % len(walks)]
        s0 = int(rng.integers(0, max(1, len(w) - list_nodes)))
        lists.append(w[s0:s0 + list_nodes].astype(np.uint32))
        bases.append((idx[lists[-1]] - idx[lists[-1] - 1]).astype(np.uint32))
    rows = []
    for n_paths in (16, 64, 256, 1024, 4096):
        span = 3000  # nodes per synthetic path: windows of the haplotypes spread over the graph
        pieces = []
        for i in range(n_paths):
            w = walks[i % len(walks)]
            s0 = (i * 7919) % max(1, len(w) - span)
            pieces.append(w[s0:s0 + span] << np.uint64(1))
        steps = np.concatenate(pieces)
        off = np.concatenate([[0], np.cumsum([len(x) for x in pieces])]).astype(np.uint64)
        t0 = time.perf_counter()
        ctx.path_support_begin(off, steps)
        begin_ms = (time.perf_counter() - t0) * 1e3
        build_ms = sum(k["ms"] for k in ctx.kernel_times() if k["name"] == "k_ps_build")
        ctx.path_support_lists(lists, bases)  # (warm-up)
        t0 = time.perf_counter()
        wb, we = ctx.path_support_lists(lists, bases)
        call_ms = (time.perf_counter() - t0) * 1e3
        score_ms = sum(k["ms"] for k in ctx.kernel_times() if k["name"] == "k_ps_score")
        rows.append({"paths": n_paths, "words_per_bitset": (n_paths + 31) // 32, "path_steps": len(steps), "begin_ms": round(begin_ms, 2),
                     "k_ps_build_ms": round(build_ms, 4), "k_ps_score_ms": round(score_ms, 4), "call_ms": round(call_ms, 2),
                     "sum_bases": int(wb.sum(dtype="uint64")), "sum_edges": int(we.sum(dtype="uint64"))})
        ctx.path_support_end()
    print(json.dumps({"graph_nodes": n_nodes, "lists": len(lists), "list_nodes": sum(len(l) for l in lists), "rows": rows}), flush=True)


def run_json(cmd, env=None, timeout=3000):
    pr = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    if pr.returncode != 0:
        raise RuntimeError("%s failed (%d): %s" % (" ".join(cmd), pr.returncode, pr.stderr[-600:]))
    return json.loads(pr.stdout.strip().splitlines()[-1])


def lib_env(parent_lib):
    env = dict(os.environ)
    env.pop("VGA_LIB", None)
    if parent_lib:
        env["VGA_LIB"] = parent_lib
    return env


def bench_ab(parent_lib, repeats):
    vals = {"branch": [], "parent": []}
    for rep in range(repeats):
        for side in (("branch", "parent") if rep % 2 == 0 else ("parent", "branch")):
            line = run_json([sys.executable, os.path.join(ROOT, "bench.py")], env=lib_env(parent_lib if side == "parent" else None))
            vals[side].append(line["value"])
            print(side, line["value"], file=sys.stderr, flush=True)
    lo_b, hi_b, lo_p, hi_p = min(vals["branch"]), max(vals["branch"]), min(vals["parent"]), max(vals["parent"])
    return {"command": "python bench.py", "metric": "aligned reads/s, config 3", "runs": vals, "branch_range": [lo_b, hi_b], "parent_range": [lo_p, hi_p],
            "ranges_overlap": bool(lo_b <= hi_p and lo_p <= hi_b), "branch_best_below_parent_worst": bool(hi_b < lo_p)}


def step(gfa, n_reads, steps, warmup, repeats):
    runs = {"off": [], "on": []}
    for rep in range(repeats):
        for s in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            runs[s].append(run_json([sys.executable, os.path.abspath(__file__), "--child", gfa, str(n_reads), str(steps), str(warmup),
                                     "1" if s == "on" else "0"], env=lib_env(None)))
            print(s, json.dumps(runs[s][-1]), file=sys.stderr, flush=True)
    mean = lambda v: sum(v) / len(v)
    rate = {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}
    on = runs["on"]
    return {"reads": n_reads, "steps": steps, "aligned_reads_per_s": rate, "ms_per_step": {s: [r["ms_per_step"] for r in runs[s]] for s in runs},
            "slowdown_on_vs_off": round(1.0 - mean(rate["on"]) / mean(rate["off"]), 4),
            "busy_ms_per_step_on": {n: round(mean([r["busy_ms_per_step"][n] for r in on]), 3) for n in BUSY},
            "begin": on[-1]["begin"], "scored": on[-1]["scored"]}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        gfa, n, steps, warmup, on = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        return child_step(gfa, n, steps, warmup, on)
    if len(sys.argv) > 1 and sys.argv[1] == "--child-many":
        return child_many(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parts", default="bench_ab,step,many")
    ap.add_argument("--repeats", type=int, default=4)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lists", type=int, default=10000)
    ap.add_argument("--list-nodes", type=int, default=400)
    a = ap.parse_args()
    import __graft_entry__ as ge

    p = ge.load_package()
    parts = a.parts.split(",")
    if "bench_ab" in parts and not a.parent_lib:
        ap.error("bench_ab compares against the parent commit: --parent-lib")
    cfg5 = os.path.join(tempfile.mkdtemp(prefix="vga_path_support_"), "config5.gfa")
    if "step" in parts or "many" in parts:
        p.readsim.synth_pangenome(cfg5)
    res = {"command": "python tests/prof_path_support.py " + " ".join(x for x in sys.argv[1:] if not x.startswith("/")), "repeats": a.repeats}
    if "bench_ab" in parts:
        res["bench_ab"] = bench_ab(os.path.abspath(a.parent_lib), a.repeats)
    if "step" in parts:
        res["step"] = {"config3": step(DRB1, a.reads, a.steps, a.warmup, a.repeats), "config5": step(cfg5, a.reads, a.steps, a.warmup, a.repeats)}
    if "many" in parts:
        res["many"] = {"config5": run_json([sys.executable, os.path.abspath(__file__), "--child-many", cfg5, str(a.lists), str(a.list_nodes)],
                                           env=lib_env(None))}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
