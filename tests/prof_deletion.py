"""diagnostic: what keeping and calling the deletion events costs.  One JSON object on stdout
(profiles/deletion_calls.json).  Every measurement runs in a child process of its own with a time limit of its own, and the sides
of a comparison alternate and take turns to run first, so that both see the same box in the same minutes; the first child that
fails ends the script.  `--parent-lib` names a libvga_hip.so built from the parent commit by the same compiler (the binding's
VGA_LIB).

  bench_ab   the switch off costs nothing: `python bench.py --gpus 1 --steps 3 --warmup 1` (config 3) with this tree's library and
             with the parent's, `--repeats` runs each; the value of every run, the ranges, and whether they overlap.
  step       config 3 steps (10 000 x 10 kbp reads: map + align, the step bench.py times) counting the pileup alone -- what
             --call-variants turns on -- and keeping the deletion store too -- --call-deletions --: aligned reads/s and, from
             vga_last_kernel_times, the busy time per step of k_pu_events, k_dl_events and k_dl_keep; the events per read.  The side
             that keeps the store then calls from it (the reads of all timed steps): vga_deletion_call's wall time and its kernels.
  seam       vga_deletion_call_table on synthetic events, 10^4, 10^6 and 10^7 of them: wall time (with the host's check of every
             event and the upload) and the kernels.

    python tests/prof_deletion.py --parent-lib PATH [--parts bench_ab,step,seam] [--repeats 3] [--reads 10000] [--steps 4]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRB1 = os.path.join(ROOT, "tests", "golden", "data", "DRB1-3123.gfa")
BUSY = ("k_pu_events", "k_pu_add", "k_dl_events", "k_dl_keep", "poa_text", "poa_band_dp")


def kernels_ms(ctx):
    return {t["name"]: round(t["ms"], 4) for t in ctx.kernel_times() if t["name"].startswith("k_dl")}


def child_step(n_reads, steps, warmup, deletions):
    """one process: reads/s of the timed steps and the kernels' busy time per step; with `deletions` the call behind them"""
    import __graft_entry__ as ge

    p = ge.load_package()
    hidx = p.HostIndex.build_from_gfa(DRB1, 11)
    ctx = p.Context(0)
    hidx.upload(ctx)
    b = ctx.batch([r.seq for r in p.readsim.config3_reads(DRB1, n_reads)])
    ctx.pileup_begin()
    if deletions:
        ctx.deletion_begin()
    for _ in range(warmup):
        b.map_align_raw()
    ctx.synchronize()
    ctx.pileup_reset()
    if deletions:
        ctx.deletion_reset()
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
    out = {"aligned_reads_per_s": round(aligned / dt, 1), "ms_per_step": round(dt / steps * 1e3, 1),
           "busy_ms_per_step": {n: round(v / steps, 3) for n, v in busy.items()}}
    if deletions:
        t1 = time.perf_counter()
        events, n_al, n_end = ctx.deletions()
        out["read_ms"] = round((time.perf_counter() - t1) * 1e3, 2)
        out["stored"] = {"alignments": n_al, "events": int(len(events)), "end_runs": n_end, "events_per_read": round(len(events) / max(n_al, 1), 1),
                         "longest": int(events[:, 1].max()) if len(events) else 0, "of_64_or_more": int((events[:, 1] >= 64).sum())}
        ctx.deletion_call()  # (warm-up)
        calls = []
        for _ in range(3):
            t1 = time.perf_counter()
            got = ctx.deletion_call()
            calls.append({"call_wall_ms": round((time.perf_counter() - t1) * 1e3, 3), "kernels_ms": kernels_ms(ctx)})
        out["call"] = {"n_distinct": got["n_distinct"], "n_calls": got["n_calls"], "vga_deletion_call": calls}
    print(json.dumps(out), flush=True)


def child_seam(n):
    import numpy as np

    import __graft_entry__ as ge

    p = ge.load_package()
    ctx = p.Context(0)
    n_bases = 100000
    rng = np.random.default_rng(n)
    pool = np.stack([rng.integers(0, n_bases, n // 4 + 1), rng.integers(1, 3000, n // 4 + 1), rng.integers(0, n_bases, n // 4 + 1)], 1)
    ev = pool[rng.integers(0, len(pool), n)].astype(np.uint32)
    tab = rng.integers(0, 8, size=(n_bases, 7)).astype(np.uint64)
    ctx.deletion_call_table(ev, tab)  # (warm-up)
    runs = []
    for _ in range(3):
        t1 = time.perf_counter()
        got = ctx.deletion_call_table(ev, tab)
        runs.append({"call_wall_ms": round((time.perf_counter() - t1) * 1e3, 3), "kernels_ms": kernels_ms(ctx)})
    print(json.dumps({"events": n, "n_bases": n_bases, "n_distinct": got["n_distinct"], "n_calls": got["n_calls"], "vga_deletion_call_table": runs}), flush=True)


def run_child(args, env=None, limit=600):
    pr = subprocess.run([sys.executable] + args, capture_output=True, text=True, timeout=limit, env=env, cwd=ROOT)
    if pr.returncode != 0:
        sys.stderr.write(pr.stdout[-2000:] + pr.stderr[-4000:])
        raise SystemExit("child failed (%d): %s" % (pr.returncode, " ".join(args)))
    print("done:", " ".join(args)[-100:], file=sys.stderr, flush=True)
    return json.loads([l for l in pr.stdout.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--parts", default="bench_ab,step,seam")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--child", nargs="*")
    a = ap.parse_args()
    if a.child:
        os.environ.setdefault("VGA_TUNE_MALLOC", "1")  # as bench.py
        if a.child[0] == "seam":
            return child_seam(int(a.child[1]))
        return child_step(int(a.child[0]), int(a.child[1]), int(a.child[2]), int(a.child[3]))
    me = os.path.abspath(__file__)
    out = {"what": "what keeping and calling the deletion events costs on one MI355X (DESIGN.md section 31); no figure here is asserted by a test"}
    parts = a.parts.split(",")
    mean = lambda v: sum(v) / len(v)
    if "bench_ab" in parts:
        assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: a libvga_hip.so built from the parent commit"
        runs, order = {"branch": [], "parent": []}, []
        for rep in range(a.repeats):
            for side in (("branch", "parent") if rep % 2 == 0 else ("parent", "branch")):
                env = dict(os.environ)
                env.pop("VGA_LIB", None)
                if side == "parent":
                    env["VGA_LIB"] = os.path.abspath(a.parent_lib)
                runs[side].append(run_child([os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], env=env)["value"])
                order.append(side)
        rng = {s: [min(v), max(v)] for s, v in runs.items()}
        out["bench_ab"] = {"bench": "python bench.py --gpus 1 --steps 3 --warmup 1", "metric": "aligned reads/s, config 3", "order": order,
                           "how": "processes of their own on one box; the parent's library built from the parent commit with the same compiler (VGA_LIB)",
                           "runs": runs, "branch_range": rng["branch"], "parent_range": rng["parent"],
                           "ranges_overlap": rng["branch"][0] <= rng["parent"][1] and rng["parent"][0] <= rng["branch"][1]}
    if "step" in parts:
        env = dict(os.environ)
        env.pop("VGA_LIB", None)
        runs = {"pileup": [], "pileup_and_deletions": []}
        for rep in range(a.repeats):
            for side in (list(runs) if rep % 2 == 0 else list(runs)[::-1]):
                runs[side].append(run_child([me, "--child", str(a.reads), str(a.steps), str(a.warmup), str(int(side != "pileup"))], env=env))
        rate = {s: [r["aligned_reads_per_s"] for r in runs[s]] for s in runs}
        on = runs["pileup_and_deletions"]
        busy = {n: round(mean([r["busy_ms_per_step"][n] for r in on]), 3) for n in BUSY}
        out["step"] = {"workload": "config 3: %d reads of 10 kbp on DRB1-3123, %d timed steps after %d" % (a.reads, a.steps, a.warmup),
                       "aligned_reads_per_s": rate, "ms_per_step": {s: [r["ms_per_step"] for r in runs[s]] for s in runs},
                       "ranges": {s: [min(v), max(v)] for s, v in rate.items()},
                       "slowdown_with_deletions": round(1.0 - mean(rate["pileup_and_deletions"]) / mean(rate["pileup"]), 4),
                       "busy_ms_per_step_keeping_the_store": busy,
                       "k_dl_events_over_k_pu_events": round(busy["k_dl_events"] / max(busy["k_pu_events"], 1e-9), 3),
                       "read_ms": [r["read_ms"] for r in on], "stored": on[-1]["stored"], "call": on[-1]["call"]}
    if "seam" in parts:
        env = dict(os.environ)
        env.pop("VGA_LIB", None)
        out["seam"] = [run_child([me, "--child", "seam", str(n)], env=env) for n in (10**4, 10**6, 10**7)]
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
