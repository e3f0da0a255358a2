"""diagnostic: what the path edit distance costs.  One JSON object on stdout (profiles/path_edit.json).
Every measurement runs in a child process of its own with a time limit of its own, and the processes of a pair alternate, so that
both sides of a comparison see the same box in the same minutes; the first child that fails ends the script.  `--parent-lib` names a
libvga_hip.so built from the parent commit by the same compiler (the binding's VGA_LIB).

  bench_ab   off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and with the
             parent's, alternating, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  seam       k_pe_dist alone through vga_path_edit_pairs: `--pairs` queries of 10 kbp with 10 % edits against texts of 16 kbp (a DRB1
             path), where the word-steps are known exactly: blocks(m) x n per pair.
  step       the on-cost: one workload step (`--reads` x 10 kbp reads: map + align, the step bench.py times) with path support on and
             with path support plus the edit distance on, same library; the kernel times of the k_pe_* kernels from
             vga_last_kernel_times, the scored pairs, and an upper bound of the word-steps (blocks(m) x min(|seq_p|, 3 m) per scored
             pair: the window is the anchor span plus 2 m).  `--workloads config3,config5`.

    python tests/prof_path_edit.py --parent-lib PATH [--parts bench_ab,seam,step] [--repeats 3] [--reads 10000] [--pairs 2000]
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
PE = ("k_pe_jobs", "k_pe_dist", "k_pe_rows")


def child_seam(n_pairs):
    import random

    import __graft_entry__ as ge

    p = ge.load_package()
    ctx = p.Context(0)
    rng = random.Random(5)
    text = "".join(rng.choice("ACGT") for _ in range(16000))
    qs = []
    for _ in range(n_pairs):
        at = rng.randrange(0, 6000)
        qs.append("".join(c if rng.random() > 0.1 else rng.choice("ACGT") for c in text[at:at + 10000]))
    ctx.path_edit_pairs(qs[:8], [text] * 8)  # (warm-up)
    t0 = time.perf_counter()
    out = ctx.path_edit_pairs(qs, [text] * n_pairs)
    wall = time.perf_counter() - t0
    k = {t["name"]: t for t in ctx.kernel_times()}
    ws = n_pairs * ((10000 + 63) // 64) * len(text)
    ms = k["k_pe_dist"]["ms"]
    print(json.dumps({"pairs": n_pairs, "query_letters": 10000, "text_letters": len(text), "blocks_per_lane": 4, "lanes": 40,
                      "k_pe_dist_ms": round(ms, 3), "k_pe_encode_ms": round(k["k_pe_encode"]["ms"], 3), "call_wall_ms": round(wall * 1e3, 1),
                      "word_steps": ws, "word_steps_per_s": round(ws / (ms * 1e-3), 0), "mean_edit": round(float(out.mean()), 1)}))
    ctx.close()


def child_step(workload, n_reads, with_edit):
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    gfa = DRB1
    if workload == "config5":
        gfa = os.path.join(tempfile.mkdtemp(prefix="vga_prof_"), "config5.gfa")
        p.readsim.synth_pangenome(gfa)
    g = p.hostlib.gfa_paths(gfa)
    n_paths = len(g["step_off"]) - 1
    if n_paths < 1:
        print(json.dumps({"workload": workload, "skipped": "the graph has no P line"}))
        return
    reads = p.readsim.simulate_reads(gfa, n_reads, 10000, 0.03, 0.03, 0.04, seed=77)
    seqs = [r.seq for r in reads]
    hidx = p.HostIndex.build_from_gfa(gfa, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    ctx.path_support_begin(g["step_off"], g["steps"])
    if with_edit:
        ctx.path_edit_begin()
    batch = ctx.batch(seqs)
    batch.map_align_raw()  # (warm-up: the pools grow)
    t0 = time.perf_counter()
    last = batch.map_align_raw()
    wall = time.perf_counter() - t0
    k = {t["name"]: t for t in last["kernels"]}
    row = {"workload": workload, "reads": n_reads, "paths": n_paths, "edit": bool(with_edit), "step_wall_ms": round(wall * 1e3, 1),
           "aligned": int(last["aligned"]), "k_ps_score_ms": round(k.get("k_ps_score", {}).get("ms", 0.0), 3)}
    if "poa_band_dp" in k:
        row["poa_band_dp_busy_ms"] = round(k["poa_band_dp"]["busy_ms"], 1)
    if with_edit:
        for name in PE:
            row[name + "_ms"] = round(k[name]["ms"], 3)
            row[name + "_launches"] = k[name]["launches"]
        e = ctx.path_edit_last(len(seqs)).astype(np.int64)
        m = np.array([len(s) for s in seqs], dtype=np.int64)
        plen = np.array([int(x) for x in g["length"]], dtype=np.int64) if "length" in g else None
        scored = e != p.binding.PATH_EDIT_NONE
        row["scored_pairs"] = int(scored.sum())
        row["too_long"] = ctx.path_edit()["n_too_long"]
        if plen is not None:
            ub = (((m + 63) // 64)[:, None] * np.minimum(plen[None, :], 3 * m[:, None]) * scored).sum()
            row["word_steps_upper_bound"] = int(ub)
            row["word_steps_per_s_upper_bound"] = round(float(ub) / (k["k_pe_dist"]["ms"] * 1e-3), 0)
        row["mean_row_minimum_over_length"] = round(float(np.mean([e[r][scored[r]].min() / m[r] for r in range(len(seqs)) if scored[r].any()])), 4)
    print(json.dumps(row))
    ctx.close()


def run_child(args, env=None, limit=600):
    pr = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if pr.returncode != 0:
        sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-4000:])
        raise SystemExit("child failed (%d): %s" % (pr.returncode, " ".join(args)))
    return json.loads([l for l in pr.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parts", default="bench_ab,seam,step")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--workloads", default="config3,config5")
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "seam":
            child_seam(int(a.child[1]))
        else:
            child_step(a.child[1], int(a.child[2]), a.child[3] == "1")
        return
    me = os.path.abspath(__file__)
    out = {"what": "what the path edit distance costs on one MI355X (DESIGN.md section 19); no figure here is asserted by a test"}
    parts = a.parts.split(",")
    if "seam" in parts:
        out["seam"] = run_child([me, "--child", "seam", str(a.pairs)])
    if "step" in parts:
        out["step"] = []
        for wl in a.workloads.split(","):
            for with_edit in ("0", "1"):
                out["step"].append(run_child([me, "--child", "step", wl, str(a.reads), with_edit], limit=900))
    if "bench_ab" in parts:
        assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: a libvga_hip.so built from the parent commit"
        runs = {"branch": [], "parent": []}
        for _ in range(a.repeats):
            for side in ("branch", "parent"):
                env = dict(os.environ)
                if side == "parent":
                    env["VGA_LIB"] = os.path.abspath(a.parent_lib)
                else:
                    env.pop("VGA_LIB", None)
                runs[side].append(run_child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env)["value"])
        rng = {s: [min(v), max(v)] for s, v in runs.items()}
        out["bench_ab"] = {"bench": "python bench.py --gpus 1 --steps 3 --warmup 1", "metric": "aligned reads/s, config 3",
                           "order": "branch and parent alternating, processes of their own, one box; the parent's library built from the parent commit with the same compiler (VGA_LIB)",
                           "runs": runs, "branch_range": rng["branch"], "parent_range": rng["parent"],
                           "ranges_overlap": rng["branch"][0] <= rng["parent"][1] and rng["parent"][0] <= rng["branch"][1]}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
